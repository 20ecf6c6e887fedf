"""The read clean-up rule restated in plain Python from its specification (DESIGN.md section 4 "Clean"), base by base — nothing of csrc/clean_core.hpp's ballots —,
and the case table the host and the GPU tests share."""
import numpy as np

DEFAULTS = dict(poly_base=ord("G"), poly_min_len=10, poly_one_in=8, poly_max_mismatch=5, min_quality=2, min_length=15, max_dust=70)
POLY, TRIM_N, TRIM_QUAL, DUST, ALL = 1, 2, 4, 8, 15
MAX_LEN = 1024
LEN_BINS, DUST_BINS = 1025, 101
KEPT, TRIMMED, TOO_SHORT, LOW_COMPLEXITY, EMPTY, TOO_LONG = range(6)
_VALID = frozenset(b"ACGT")


def poly_tail(r, P):
    L, x, tail = len(r), 0, 0
    for n in range(1, L + 1):
        x += r[L - n] != P["poly_base"]
        if x > P["poly_max_mismatch"] or (n >= P["poly_min_len"] and x * P["poly_one_in"] > n):
            break
        if n >= P["poly_min_len"] and r[L - n] == P["poly_base"]:
            tail = n
    return tail


def removable(b, q, ops, P):
    return bool((ops & TRIM_N and b not in _VALID) or (ops & TRIM_QUAL and q != 255 and q <= P["min_quality"]))


def window_score(w):
    counts = {}
    for i in range(len(w) - 2):
        t = bytes(w[i:i + 3])
        if all(b in _VALID for b in t):
            counts[t] = counts.get(t, 0) + 1
    T = sum(counts.values())
    S = sum(c * (c - 1) // 2 for c in counts.values())
    return 0 if T < 2 else 2000 * S // (T * (T - 1))


def dust_score(r):
    M, k, best = len(r), 0, 0
    while True:
        best = max(best, window_score(r[32 * k:min(32 * k + 64, M)]))
        if 32 * k + 64 >= M:
            return best
        k += 1


def clean_read(r, q, ops, P=DEFAULTS):
    """(class, trim5, trim3, poly_len, dust, bases, quals) of one read"""
    L = len(r)
    if L == 0:
        return EMPTY, 0, 0, 0, 0, b"", b""
    if L > MAX_LEN:
        return TOO_LONG, 0, 0, 0, 0, bytes(r), bytes(q)
    poly = poly_tail(r, P) if ops & POLY else 0
    lo, hi = 0, L - poly
    while hi > lo and removable(r[hi - 1], q[hi - 1], ops, P):
        hi -= 1
    while lo < hi and removable(r[lo], q[lo], ops, P):
        lo += 1
    M = hi - lo
    if M < P["min_length"]:
        return TOO_SHORT, lo, L - hi, poly, 0, b"", b""
    dust = dust_score(r[lo:hi]) if ops & DUST else 0
    if ops & DUST and dust > P["max_dust"]:
        return LOW_COMPLEXITY, lo, L - hi, poly, dust, b"", b""
    return (TRIMMED if M < L else KEPT), lo, L - hi, poly, dust, bytes(r[lo:hi]), bytes(q[lo:hi])


def run_rule(reads, ops, P=DEFAULTS):
    """the rule over a list of reads [(bases, quals)] in the layout of a mapad_clean_result_t"""
    n = len(reads)
    out = {"cls": np.zeros(n, np.uint8), "trim5": np.zeros(n, np.uint16), "trim3": np.zeros(n, np.uint16), "poly_len": np.zeros(n, np.uint16), "dust": np.zeros(n, np.uint16),
           "offsets": np.zeros(n + 1, np.uint64)}
    counts = {"reads_seen": n, "class_counts": np.zeros(6, np.uint64), "bases_in": 0, "bases_out": 0, "bases_poly": 0, "bases_trim5": 0, "bases_trim3": 0,
              "length_histogram": np.zeros(LEN_BINS, np.uint64), "dust_histogram": np.zeros(DUST_BINS, np.uint64)}
    bases, quals = bytearray(), bytearray()
    for i, (r, q) in enumerate(reads):
        cls, t5, t3, poly, dust, b, y = clean_read(r, q, ops, P)
        out["cls"][i], out["trim5"][i], out["trim3"][i], out["poly_len"][i], out["dust"][i] = cls, t5, t3, poly, dust
        bases += b
        quals += y
        out["offsets"][i + 1] = len(bases)
        counts["class_counts"][cls] += 1
        counts["bases_in"] += len(r)
        counts["bases_out"] += len(b)
        counts["bases_poly"] += poly
        counts["bases_trim5"] += t5
        counts["bases_trim3"] += t3 - poly
        if cls in (KEPT, TRIMMED, TOO_LONG) and len(b) < LEN_BINS:
            counts["length_histogram"][len(b)] += 1
        if ops & DUST and cls in (KEPT, TRIMMED, LOW_COMPLEXITY):
            counts["dust_histogram"][dust // 10] += 1
    out["seqs"], out["quals"], out["counts"] = np.frombuffer(bytes(bases), np.uint8), np.frombuffer(bytes(quals), np.uint8), counts
    return out


def pack(reads):
    """[(bases, quals)] -> seqs, quals, offsets as mapad_map_batch takes them"""
    offsets = np.zeros(len(reads) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(r) for r, _ in reads])
    seqs = np.frombuffer(b"".join(bytes(r) for r, _ in reads), np.uint8)
    quals = np.frombuffer(b"".join(bytes(q) for _, q in reads), np.uint8)
    return seqs, quals, offsets


PER_READ = ("cls", "trim5", "trim3", "poly_len", "dust", "offsets", "seqs", "quals")
COUNTERS = ("reads_seen", "bases_in", "bases_out", "bases_poly", "bases_trim5", "bases_trim3")


def assert_same(got, want, what=""):
    for k in PER_READ:
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs at {np.flatnonzero(np.asarray(got[k][:len(want[k])]) != np.asarray(want[k][:len(got[k])]))[:8]}"
    for k in COUNTERS:
        assert int(got["counts"][k]) == int(want["counts"][k]), f"{what}: {k}"
    for k in ("class_counts", "length_histogram", "dust_histogram"):
        assert np.array_equal(got["counts"][k], want["counts"][k]), f"{what}: {k}"


# ---- synthetic reads -----------------------------------------------------------------------------------------------------------------------------------------
def rand_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())


def q30(n):
    return bytes([30]) * n


def no_g_end(rng, n):
    """n random bases whose last is not G: what stands in front of a planted tail"""
    s = bytearray(rand_bases(rng, n))
    if n and s[-1] == ord("G"):
        s[-1] = ord("A")
    return bytes(s)


def tail_with(n, mismatches=()):
    """n G with another base at the given 1-based positions counted from the 3' end"""
    t = bytearray(b"G" * n)
    for m in mismatches:
        t[n - m] = ord("A")
    return bytes(t)


# ---- the case table ------------------------------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 3, 14, 15, 63, 64, 65, 95, 96, 97, 128, 1023, 1024, 1025]
TAILS = [9, 10, 11, 63, 64, 65, 130]


def _shapes(rng):
    reads = []
    # the lengths: random reads, and the same lengths as one poly tail (the tail that is the whole read), as one homopolymer of A, as all N
    for L in LENGTHS:
        reads += [(rand_bases(rng, L), q30(L)), (b"G" * L, q30(L)), (b"A" * L, q30(L)), (b"N" * L, q30(L))]
    # planted tails behind a non-G base, with and without qualities
    for n in TAILS:
        for body in (0, 1, 20, 64 - n % 64, 200):
            reads.append((no_g_end(rng, body) + b"G" * n, q30(body + n)))
        reads.append((no_g_end(rng, 40) + b"G" * n, bytes([255]) * (40 + n)))
    body = no_g_end(rng, 50)
    # the allowed mismatch as the 8th and as the 16th base of the tail (one other base in eight), one too early (the 7th), a sixth mismatch in a long tail
    reads += [(body + tail_with(30, m), q30(80)) for m in ((8,), (16,), (8, 16), (7,), (8, 15), (8, 16, 24), (9,), (10,))]
    reads.append((body + tail_with(100, (8, 16, 24, 32, 40)), q30(150)))
    reads.append((body + tail_with(100, (8, 16, 24, 32, 40, 48)), q30(150)))
    reads.append((body + tail_with(100, (8, 16, 24, 32, 40, 60)), q30(150)))
    # the stop on the last lane of a trip (n = 64, 128) and on the first lane of the next (n = 65, 129): a run of other bases in front of a tail of n - 1
    for n in (64, 65, 128, 129):
        reads.append((rand_bases(rng, 30) + b"ACTA" + b"G" * (n - 1), q30(33 + n)))
        reads.append((b"T" * 40 + b"G" * (n - 1), q30(39 + n)))
        reads.append((b"T" * 40 + tail_with(n - 1, (8, 16, 24, 32, 40)), q30(39 + n)))
    # a tail that begins with a non-G: the cut is at the first G behind it
    reads += [(body + b"A" + b"G" * 12, q30(63)), (body + b"AAGAG" + b"G" * 12, q30(67)), (body + b"G" * 12 + b"A", q30(63)), (body + b"G" * 12 + b"AC", q30(64))]
    # qualities 0, 2, 3 and 255 at both ends; N at the ends; N and a low quality inside
    core = rand_bases(rng, 40)
    for v in (0, 2, 3, 255):
        for k in (1, 3):
            reads.append((rand_bases(rng, k) + core + rand_bases(rng, k), bytes([v]) * k + q30(40) + bytes([v]) * k))
            reads.append((core + rand_bases(rng, k), q30(40) + bytes([v]) * k))
            reads.append((rand_bases(rng, k) + core, bytes([v]) * k + q30(40)))
    reads += [(b"NN" + core + b"N", q30(43)), (b"N" + core[:20] + b"N" + core[20:] + b"NNN", q30(45)), (core, q30(20) + bytes([0]) + q30(19)),
              (b"R" + core + b"y", q30(42)), (b"N" * 70 + core + b"N" * 70, q30(180)), (core + b"N" * 64, q30(104)), (b"N" * 64 + core, q30(104)),
              (b"N" * 63 + core + b"N" * 65, q30(168))]
    # ends that meet: every base removable by quality, by N, by one of each; the meeting point at a trip's edge
    reads += [(rand_bases(rng, 50), bytes([2]) * 50), (rand_bases(rng, 64), bytes([0]) * 64), (rand_bases(rng, 65), bytes([1]) * 65), (rand_bases(rng, 130), bytes([2]) * 130),
              (b"N" * 20 + rand_bases(rng, 20), q30(20) + bytes([2]) * 20), (rand_bases(rng, 20) + b"N" * 20, bytes([2]) * 20 + q30(20))]
    # a poly tail in front of which low qualities and N stand: all steps on one read
    reads += [(b"N" + core + b"NN" + b"G" * 15, bytes([30]) + q30(40) + bytes([2, 2]) + q30(15)), (core[:14] + b"G" * 20, q30(34)), (core[:15] + b"G" * 20, q30(35)),
              (b"N" + core[:15] + b"N" + b"G" * 20, q30(37)), (b"N" + core[:14] + b"N" + b"G" * 20, q30(36))]
    # complexity: repeats of period 1 to 4 at the lengths around the windows; a window with T = 0 and one with T = 1; N inside a window
    for unit in (b"A", b"AC", b"ACG", b"ACGT", b"AAC", b"GGT"):
        for L in (15, 16, 63, 64, 65, 95, 96, 97, 128, 200):
            reads.append(((unit * L)[:L], q30(L)))
    reads += [(b"ANN" * 10, q30(30)), (b"ACG" + b"N" * 27, q30(30)), (b"NNACGNN" + b"N" * 23, q30(30)), (b"ACGT" + b"N" * 26, q30(30)), (b"A" * 30 + b"N" + b"A" * 30, q30(61)),
              ((b"AN" * 32), q30(64)), (b"A" * 20 + b"N" * 30 + b"C" * 20, q30(70))]
    # a repeat confined to the last, short window of a 97-base read (bases 64 .. 96), to the middle window alone, to the first 32 bases alone
    r96 = rand_bases(rng, 97)
    reads += [(r96[:64] + b"A" * 33, q30(97)), (r96[:64] + (b"AC" * 17)[:33], q30(97)), (r96[:80] + b"A" * 17, q30(97)), (r96[:32] + b"T" * 32 + r96[64:], q30(97)),
              (b"C" * 32 + r96[32:], q30(97)), (r96, q30(97)), (r96[:90] + b"A" * 7, q30(97))]
    # long reads: a repeat deep inside 1024 bases, a tail of 130 behind 894
    big = rand_bases(rng, 1024)
    reads += [(big[:700] + b"AT" * 40 + big[780:], q30(1024)), (no_g_end(rng, 894) + b"G" * 130, q30(1024)), (b"N" * 500 + big[:24] + b"N" * 500, q30(1024)),
              (big + b"G", q30(1025)), (b"A" * 1025, q30(1025))]
    return reads


def case_table(seed=17):
    """[(label, ops, params, [(bases, quals)])]: one set of shapes under every op alone, all ops together and other parameters"""
    reads = _shapes(np.random.default_rng(seed))
    groups = [(name, ops, DEFAULTS, reads) for name, ops in (("poly alone", POLY), ("trim_n alone", TRIM_N), ("trim_qual alone", TRIM_QUAL), ("dust alone", DUST),
                                                              ("no op: the length test", 0), ("both ends", TRIM_N | TRIM_QUAL), ("all ops", ALL))]
    groups.append(("all ops, other parameters", ALL, dict(poly_base=ord("A"), poly_min_len=1, poly_one_in=1, poly_max_mismatch=0, min_quality=0, min_length=0, max_dust=0), reads))
    groups.append(("all ops, loose parameters", ALL, dict(poly_base=ord("G"), poly_min_len=20, poly_one_in=4, poly_max_mismatch=40, min_quality=20, min_length=3, max_dust=1000),
                   reads))
    groups.append(("all ops, dust 320", ALL, dict(DEFAULTS, max_dust=320, min_length=1), reads))
    return groups


def mixed_reads(n, seed):
    """reads of 20 .. 160 bases of every kind: random, with a planted tail, with bad ends, repeats; qualities of 0 .. 41 and some reads without"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.integers(20, 161))
        r = bytearray(rand_bases(rng, L))
        q = bytearray(rng.integers(0, 42, L, dtype=np.uint8).tobytes())
        kind = i % 5
        if kind == 1:
            t = int(rng.integers(5, min(L, 80)))
            r[L - t:] = b"G" * t
            for p in rng.integers(0, L, 2):
                r[p] = rng.choice(np.frombuffer(b"ACGTN", np.uint8))
        elif kind == 2:
            a, b = int(rng.integers(0, 6)), int(rng.integers(0, 6))
            r[:a] = b"N" * a
            q[L - b:] = bytes(b)
        elif kind == 3:
            unit = rand_bases(rng, int(rng.integers(1, 5)))
            a = int(rng.integers(0, L // 2))
            r[a:] = (unit * L)[:L - a]
        elif kind == 4 and i % 10 == 4:
            q = bytearray([255]) * L
        out.append((bytes(r), bytes(q)))
    return out


# ---- what the command-line tests share -------------------------------------------------------------------------------------------------------------------------
def _mu():
    import merge_util
    return merge_util


def write_fastq(path, names, reads):
    import gzip
    text = "".join(f"@{n}\n{r.decode()}\n+\n{''.join(chr(33 + v) for v in q)}\n" for n, (r, q) in zip(names, reads))
    with (gzip.open(path, "wt") if str(path).endswith(".gz") else open(path, "w")) as f:
        f.write(text)


def read_fastq(path):
    import gzip
    with (gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)) as f:
        lines = f.read().split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % 4 == 0
    return [(lines[i][1:], lines[i + 1].encode(), bytes(ord(c) - 33 for c in lines[i + 3])) for i in range(0, len(lines) - 1, 4)]


def cli_reads(n, seed):
    """mixed reads as a FASTQ file can hold them: a read without qualities (255) gets 30"""
    return [(r, bytes(30 if v == 255 else v for v in q)) for r, q in mixed_reads(n, seed)]


def expected_records(want, names):
    out = []
    for i, name in enumerate(names):
        if want["cls"][i] in (KEPT, TRIMMED, TOO_LONG):
            b, e = int(want["offsets"][i]), int(want["offsets"][i + 1])
            out.append((name, want["seqs"][b:e].tobytes(), want["quals"][b:e].tobytes()))
    return out


def read_report(path):
    """the three sections of a --clean_report file: {key: value}, {length: count}, {dust: count}; the format is asserted on the way"""
    rows = [ln.split("\t") for ln in open(path).read().splitlines()]
    assert all(len(r) == 2 for r in rows)
    at_len = next(i for i, r in enumerate(rows) if r[0] == "length_histogram")
    at_dust = next(i for i, r in enumerate(rows) if r[0] == "dust_histogram")
    keys = {k: int(v) for k, v in rows[:at_len]}
    assert at_dust == at_len + 1 + int(rows[at_len][1]) and len(rows) == at_dust + 1 + int(rows[at_dust][1])
    lengths = {int(k): int(v) for k, v in rows[at_len + 1:at_dust]}
    dust = {int(k): int(v) for k, v in rows[at_dust + 1:]}
    assert list(lengths) == sorted(lengths) and list(dust) == sorted(dust) and all(k % 10 == 0 for k in dust)
    return keys, lengths, dust


def check_report(path, want):
    keys, lengths, dust = read_report(path)
    c = want["counts"]
    assert [keys[k] for k in ("kept", "trimmed", "too_short", "low_complexity", "empty", "too_long")] == c["class_counts"].tolist()
    for k in COUNTERS:
        assert keys[k] == c[k], k
    assert lengths == {k: int(v) for k, v in enumerate(c["length_histogram"]) if v}
    assert dust == {10 * k: int(v) for k, v in enumerate(c["dust_histogram"]) if v}
    return keys


def expected_merge_with_clean(pairs, names, ops, P=DEFAULTS):
    """what `merge` and `map --reads2` do with the clean-up options: poly-G tails off both mates as sequenced (no mate dropped), the merge rule, then the other
    steps on the merged reads.  [(name, bases, quals)], the counts of the pass over the mates and of the pass over the merged reads"""
    if ops & POLY:
        front = dict(P, min_length=0)
        m1 = run_rule([(p[0], p[1]) for p in pairs], POLY, front)
        m2 = run_rule([(p[2], p[3]) for p in pairs], POLY, front)
        cut = lambda m, i: (m["seqs"][int(m["offsets"][i]):int(m["offsets"][i + 1])].tobytes(), m["quals"][int(m["offsets"][i]):int(m["offsets"][i + 1])].tobytes())  # noqa: E731
        pairs = [cut(m1, i) + cut(m2, i) for i in range(len(pairs))]
        front_counts = {k: m1["counts"][k] + m2["counts"][k] for k in ("reads_seen", "bases_in", "bases_poly")}
        front_counts["trimmed"] = int(m1["counts"]["class_counts"][TRIMMED] + m2["counts"]["class_counts"][TRIMMED])
    else:
        front_counts = None
    merged = _mu().run_rule(pairs)
    recs = [(names[i], merged["seqs"][int(merged["offsets"][i]):int(merged["offsets"][i + 1])].tobytes(),
             merged["quals"][int(merged["offsets"][i]):int(merged["offsets"][i + 1])].tobytes()) for i in range(len(pairs)) if merged["cls"][i] == _mu().MERGED]
    back = run_rule([(b, q) for _, b, q in recs], ops & ~POLY, P)
    return expected_records(back, [n for n, _, _ in recs]), front_counts, back


def tailed_pairs(n, seed, genome=None):
    """pairs off fragments of 20 .. 150 bases (of the genome, if given), mates of 80; a third of the mates end in a poly-G tail of 10 .. 40 bases that stands in
    the place of their last bases, some fragments are repeats, some mates have bad ends"""
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(n):
        F = int(rng.integers(20, 151))
        if genome is None:
            frag = rand_bases(rng, F)
        else:
            at = int(rng.integers(0, len(genome) - F))
            frag = genome[at:at + F].tobytes()
        if i % 9 == 0:
            frag = (rand_bases(rng, int(rng.integers(1, 4))) * F)[:F]
        r1, q1, r2, q2 = _mu().sequence_pair(rng, frag, 80, 80, qual=(3, 40))
        mates = []
        for r, q in ((r1, q1), (r2, q2)):
            r, q = bytearray(r), bytearray(q)
            if rng.random() < 0.33:
                t = int(rng.integers(10, 41))
                r[80 - t:] = b"G" * t
                q[80 - t:] = bytes([37]) * t
            if rng.random() < 0.2:
                a = int(rng.integers(1, 5))
                r[:a] = b"N" * a
                q[:a] = bytes([2]) * a
            mates.append((bytes(r), bytes(q)))
        pairs.append(mates[0] + mates[1])
    return pairs
