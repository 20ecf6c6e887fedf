"""The trim-and-merge rule restated in plain Python from its specification (DESIGN.md section 4 "Trim and merge"), byte by byte and candidate by candidate —
nothing of csrc/merge_core.hpp's bit planes —, and the case table the host and the GPU tests share."""
import numpy as np

A1 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
A2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
DEFAULTS = dict(min_overlap=11, min_adapter_overlap=3, max_mismatch_permille=166, min_length=15, max_quality=41, adapter1=A1, adapter2=A2)
MAX_MATE = 512
HIST_BINS = 1025
MERGED, TOO_SHORT, UNMERGED, EMPTY_MATE, TOO_LONG = range(5)
_COMP = {65: 84, 84: 65, 67: 71, 71: 67}  # A<->T, C<->G
_VALID = frozenset(b"ACGT")


def comp(b):
    return _COMP.get(b, b)


def revcomp(s):
    return bytes(comp(b) for b in reversed(s))


def _count(pairs):
    m = x = 0
    for a, b in pairs:
        if a in _VALID and b in _VALID:
            if a == b:
                m += 1
            else:
                x += 1
    return m, x


def candidate(r1, r2, a1, a2, F):
    """(m, x) of fragment length F"""
    L1, L2 = len(r1), len(r2)
    cols = [(r1[p], comp(r2[F - 1 - p])) for p in range(max(0, F - L2), min(F, L1))]
    if F < L1:
        cols += [(r1[F + k], a1[k]) for k in range(min(L1 - F, len(a1)))]
    if F < L2:
        cols += [(r2[F + k], a2[k]) for k in range(min(L2 - F, len(a2)))]
    return _count(cols)


def choose(r1, r2, a1, a2, min_overlap, permille):
    """(F, m, x) of the admissible candidate with the greatest m - x, the smallest F among equals; None if there is none"""
    best = None
    for F in range(0, len(r1) + len(r2) - min_overlap + 1):
        m, x = candidate(r1, r2, a1, a2, F)
        n = m + x
        if n >= min_overlap and x * 1000 <= n * permille and (best is None or m - x > best[1] - best[2]):
            best = (F, m, x)
    return best


def merged_read(r1, q1, r2, q2, F, max_quality):
    L1, L2 = len(r1), len(r2)
    lo, hi = max(0, F - L2), min(F, L1)
    bases, quals = bytearray(), bytearray()
    for p in range(F):
        if p < lo:
            b, q = r1[p], q1[p]
        elif p >= hi:
            b, q = comp(r2[F - 1 - p]), q2[F - 1 - p]
        else:
            b1, b2, y1, y2 = r1[p], comp(r2[F - 1 - p]), q1[p], q2[F - 1 - p]
            h1, h2 = (0 if y1 == 255 else y1), (0 if y2 == 255 else y2)
            v1, v2 = b1 in _VALID, b2 in _VALID
            if not v1 and not v2:
                b, q = ord("N"), 0
            elif not v2:
                b, q = b1, y1
            elif not v1:
                b, q = b2, y2
            elif b1 == b2:
                b, q = b1, min(h1 + h2, max_quality)
            elif h1 == h2:
                b, q = ord("N"), 0
            elif h1 > h2:
                b, q = b1, h1 - h2
            else:
                b, q = b2, h2 - h1
            if y1 == 255 and y2 == 255:
                q = 255
        bases.append(b)
        quals.append(q)
    return bytes(bases), bytes(quals)


def merge_pair(r1, q1, r2, q2, P=DEFAULTS):
    """(class, F or -1, m, x, bases, quals) of one pair"""
    if len(r1) == 0 or len(r2) == 0:
        return EMPTY_MATE, -1, 0, 0, b"", b""
    if len(r1) > MAX_MATE or len(r2) > MAX_MATE:
        return TOO_LONG, -1, 0, 0, b"", b""
    c = choose(r1, r2, P["adapter1"], P["adapter2"], P["min_overlap"], P["max_mismatch_permille"])
    if c is None:
        return UNMERGED, -1, 0, 0, b"", b""
    F, m, x = c
    if F < P["min_length"]:
        return TOO_SHORT, F, m, x, b"", b""
    return (MERGED, F, m, x) + merged_read(r1, q1, r2, q2, F, P["max_quality"])


def trim_read(r1, q1, P=DEFAULTS):
    """single-end: mate 2 and A2 absent, min_adapter_overlap in min_overlap's place; class 0 trimmed, 2 untouched; what is left is too_short below min_length"""
    if len(r1) == 0:
        return EMPTY_MATE, -1, 0, 0, b"", b""
    if len(r1) > MAX_MATE:
        return TOO_LONG, -1, 0, 0, b"", b""
    c = choose(r1, b"", P["adapter1"], b"", P["min_adapter_overlap"], P["max_mismatch_permille"])
    F, m, x = c if c else (-1, 0, 0)
    left = F if c else len(r1)
    if left < P["min_length"]:
        return TOO_SHORT, F, m, x, b"", b""
    return (MERGED if c else UNMERGED), F, m, x, bytes(r1[:left]), bytes(q1[:left])


def run_rule(pairs, P=DEFAULTS, single=False):
    """the rule over a list of pairs [(r1, q1, r2, q2)] (single-end: [(r1, q1)]) in the layout of a mapad_merge_result_t"""
    n = len(pairs)
    out = {"cls": np.zeros(n, np.uint8), "frag_len": np.zeros(n, np.int32), "matches": np.zeros(n, np.uint16), "mismatches": np.zeros(n, np.uint16),
           "offsets": np.zeros(n + 1, np.uint64)}
    counts = {"pairs_seen": n, "class_counts": np.zeros(5, np.uint64), "bases_in": 0, "bases_out": 0, "histogram": np.zeros(HIST_BINS, np.uint64)}
    bases, quals = bytearray(), bytearray()
    for i, pr in enumerate(pairs):
        cls, F, m, x, b, q = trim_read(pr[0], pr[1], P) if single else merge_pair(pr[0], pr[1], pr[2], pr[3], P)
        out["cls"][i], out["frag_len"][i], out["matches"][i], out["mismatches"][i] = cls, F, m, x
        bases += b
        quals += q
        out["offsets"][i + 1] = len(bases)
        counts["class_counts"][cls] += 1
        counts["bases_in"] += len(pr[0]) + (0 if single else len(pr[2]))
        counts["bases_out"] += len(b)
        if cls == MERGED or (single and cls == UNMERGED):
            counts["histogram"][len(b)] += 1
    out["seqs"], out["quals"], out["counts"] = np.frombuffer(bytes(bases), np.uint8), np.frombuffer(bytes(quals), np.uint8), counts
    return out


def pack(reads):
    """[(bases, quals)] -> seqs, quals, offsets as mapad_map_batch takes them"""
    offsets = np.zeros(len(reads) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(r) for r, _ in reads])
    seqs = np.frombuffer(b"".join(bytes(r) for r, _ in reads), np.uint8)
    quals = np.frombuffer(b"".join(bytes(q) for _, q in reads), np.uint8)
    return seqs, quals, offsets


def assert_same(got, want, what=""):
    for k in ("cls", "frag_len", "matches", "mismatches", "offsets", "seqs", "quals"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs at {np.flatnonzero(np.asarray(got[k][:len(want[k])]) != np.asarray(want[k][:len(got[k])]))[:8]}"
    for k in ("pairs_seen", "bases_in", "bases_out"):
        assert int(got["counts"][k]) == int(want["counts"][k]), f"{what}: {k}"
    assert np.array_equal(got["counts"]["class_counts"], want["counts"]["class_counts"]), f"{what}: class counts"
    assert np.array_equal(got["counts"]["histogram"], want["counts"]["histogram"]), f"{what}: histogram"


# ---- synthetic pairs ---------------------------------------------------------------------------------------------------------------------------------------
def rand_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())


def sequence_pair(rng, frag, L1, L2, a1=A1, a2=A2, qual=(2, 41)):
    """what a sequencer reads off fragment `frag` with adapters a1 / a2 behind it: mates of L1 / L2 bases (adapter, then random bases, past the fragment)"""
    t1 = frag + a1 + rand_bases(rng, L1)
    t2 = revcomp(frag) + a2 + rand_bases(rng, L2)
    q1 = bytes(rng.integers(qual[0], qual[1] + 1, L1, dtype=np.uint8).tobytes())
    q2 = bytes(rng.integers(qual[0], qual[1] + 1, L2, dtype=np.uint8).tobytes())
    return t1[:L1], q1, t2[:L2], q2


def mutate(rng, s, rate):
    s = bytearray(s)
    for i in np.flatnonzero(rng.random(len(s)) < rate):
        s[i] = rng.choice([c for c in b"ACGT" if c != s[i]])
    return bytes(s)


# ---- the case table ------------------------------------------------------------------------------------------------------------------------------------------
LENGTHS = [(1, 1), (11, 11), (12, 40), (31, 33), (32, 32), (33, 31), (63, 65), (64, 64), (65, 63), (70, 70), (100, 100), (127, 129), (150, 75), (512, 512), (513, 20), (0, 30)]
FULL_SWEEP = [(32, 32), (64, 64), (65, 63), (70, 70)]


def _frag_lengths(L1, L2):
    if (L1, L2) in FULL_SWEEP:
        return list(range(0, L1 + L2 + 1))
    want = [0, 1, 10, 11, 12, L1 - 1, L1, L1 + 1, L1 + L2 - 12, L1 + L2 - 11, L1 + L2 - 10]
    return sorted({f for f in want if 0 <= f <= L1 + L2})


def _plant(rng, pair, F, cols):
    """substitutions in mate 1 at overlap columns `cols` (positions of the fragment that both mates cover)"""
    r1, q1, r2, q2 = pair
    r1 = bytearray(r1)
    lo, hi = max(0, F - len(r2)), min(F, len(r1))
    for c in cols:
        p = lo + c
        if lo <= p < hi:
            r1[p] = rng.choice([b for b in b"ACGT" if b != r1[p]])
    return bytes(r1), q1, r2, q2


def case_table(seed=7):
    """[(label, params, [(r1, q1, r2, q2)])]: groups of pairs under one parameter set each"""
    rng = np.random.default_rng(seed)
    groups = []
    base = []
    for L1, L2 in LENGTHS:
        for F in _frag_lengths(L1, L2):
            base.append(sequence_pair(rng, rand_bases(rng, F), L1, L2))
    groups.append(("lengths x fragment lengths", DEFAULTS, base))

    mm = []
    for L1, L2, F in [(70, 70, 70), (100, 100, 90), (127, 129, 130), (150, 75, 140), (65, 63, 66)]:
        pr = sequence_pair(rng, rand_bases(rng, F), L1, L2)
        n_ov = min(F, L1) - max(0, F - L2)
        for cols in ([0], [31], [32], [63], [64], [n_ov - 1], [0, 31, 32, 63, 64, n_ov - 1]):
            mm.append(_plant(rng, pr, F, cols))
    # the admissibility edge: fragments as long as both mates (no adapter columns), so that n = the overlap and x = the planted substitutions
    for L in (40, 64, 70, 100):
        edge = L * 166 // 1000
        for x in (edge, edge + 1):
            pr = sequence_pair(rng, rand_bases(rng, L), L, L)
            mm.append(_plant(rng, pr, L, list(range(0, 2 * x, 2))))
    groups.append(("mismatches", DEFAULTS, mm))

    inv = []
    for L1, L2, F in [(70, 70, 60), (70, 70, 100), (100, 100, 150)]:
        lo, hi = max(0, F - L2), min(F, L1)
        # positions inside the overlap (one column: p1 in mate 1 faces F - 1 - p1 in mate 2) and outside it.  Outside, for mate 1: its own part of the merged
        # read (p < lo; F > L2) or its adapter region (p >= F; F < L1); for mate 2: its own part of the merged read (k < F - L1: output position F - 1 - k >= L1,
        # "an invalid byte unchanged") or its adapter region (k >= F)
        p1_in = (lo + hi) // 2
        p2_in = F - 1 - p1_in
        p1_out = [p for p in (0, lo - 1) if p < lo] + [p for p in (F, L1 - 1) if F <= p < L1]
        p2_out = [k for k in (0, F - L1 - 1) if k < F - L1] + [k for k in (F, L2 - 1) if F <= k < L2]
        assert lo <= p1_in < hi and 0 <= p2_in < L2 and p1_out and p2_out
        spots = [((p1_in,), ()), ((), (p2_in,)), ((p1_in,), (p2_in,))]
        spots += [((p,), ()) for p in p1_out] + [((), (k,)) for k in p2_out] + [((p1_out[0],), (p2_out[0],)), (tuple(p1_out), tuple(p2_out))]
        for letter in (b"N", b"R"):
            for at1, at2 in spots:
                r1, q1, r2, q2 = sequence_pair(rng, rand_bases(rng, F), L1, L2)
                r1, r2 = bytearray(r1), bytearray(r2)
                for p in at1:
                    r1[p] = letter[0]
                for k in at2:
                    r2[k] = letter[0]
                inv.append((bytes(r1), q1, bytes(r2), q2))
    inv.append((b"N" * 40, bytes([30]) * 40, b"N" * 40, bytes([30]) * 40))
    groups.append(("invalid bytes", DEFAULTS, inv))

    ql = []
    for F in (50, 70, 90):
        r1, q1, r2, q2 = _plant(rng, sequence_pair(rng, rand_bases(rng, F), 70, 70), F, [3, 10, 20])
        for v1, v2 in [(30, 30), (0, 0), (41, 41), (93, 93), (93, 2), (255, 20), (20, 255), (255, 255), (0, 255)]:
            ql.append((r1, bytes([v1]) * 70, r2, bytes([v2]) * 70))
        mixed1, mixed2 = bytearray(q1), bytearray(q2)
        mixed1[::3] = bytes([255]) * len(mixed1[::3])
        mixed2[::5] = bytes([255]) * len(mixed2[::5])
        ql.append((r1, bytes(mixed1), r2, bytes(mixed2)))
    groups.append(("qualities", DEFAULTS, ql))

    q30 = bytes([30]) * 40
    ties = [(b"A" * 40, q30, b"T" * 40, q30), (b"AC" * 20, q30, b"GT" * 20, q30)]
    ties.append(sequence_pair(rng, A1[:12] + rand_bases(rng, 48), 70, 70))
    ties.append(sequence_pair(rng, A1[:12] + rand_bases(rng, 18), 70, 70))
    groups.append(("ties", DEFAULTS, ties))

    for la in (0, 1, 33, 64):
        a1, a2 = rand_bases(rng, la), rand_bases(rng, la)
        P = dict(DEFAULTS, adapter1=a1, adapter2=a2)
        prs = [sequence_pair(rng, rand_bases(rng, F), L1, L2, a1, a2) for L1, L2 in [(70, 70), (65, 63), (150, 75)] for F in (0, 5, 20, 40, 64, 70, 100, 128)]
        groups.append((f"adapters of {la}", P, prs))

    for P in (dict(DEFAULTS, min_overlap=1), dict(DEFAULTS, min_overlap=30), dict(DEFAULTS, max_mismatch_permille=0), dict(DEFAULTS, max_mismatch_permille=1000)):
        prs = []
        for L1, L2 in [(1, 1), (33, 31), (70, 70)]:
            for F in sorted({0, 1, 20, L1, L1 + L2 - 31, L1 + L2 - 30, L1 + L2 - 29, L1 + L2 - 1, L1 + L2} & set(range(0, L1 + L2 + 1))):
                pr = sequence_pair(rng, rand_bases(rng, F), L1, L2)
                prs += [pr, _plant(rng, pr, F, [1])]
        groups.append((f"min_overlap {P['min_overlap']}, permille {P['max_mismatch_permille']}", P, prs))
    return groups


def single_table(seed=11):
    """[(label, params, [(r1, q1)])] for the single-end mode"""
    rng = np.random.default_rng(seed)
    groups = []
    for la in (0, 1, 33, 64):
        a1 = A1 if la == 33 else rand_bases(rng, la)
        reads = []
        for L in (1, 2, 3, 14, 15, 16, 63, 64, 65, 100, 128, 129, 512, 513, 0):
            for F in sorted({0, 1, 14, 15, 16, L - 4, L - 3, L - 2, L - 1, L, L + 5, 63, 64, 65} & set(range(0, L + 6))):
                r1, q1, _, _ = sequence_pair(rng, rand_bases(rng, F), L, 1, a1, b"")
                reads.append((r1, q1))
                if L >= 20:
                    reads.append((mutate(rng, r1, 0.05), q1))
        reads.append((b"N" * 30, bytes([255]) * 30))
        for P in (dict(DEFAULTS, adapter1=a1), dict(DEFAULTS, adapter1=a1, min_adapter_overlap=8), dict(DEFAULTS, adapter1=a1, min_adapter_overlap=1, max_mismatch_permille=0)):
            groups.append((f"adapter of {la}, min_adapter_overlap {P['min_adapter_overlap']}", P, reads))
    return groups
