"""The SNP panel computed independently of the product: strand-split A/C/G/T counts per panel row, the read and column counters, the call rule with its mixer
and the row statistics, from what a BAM record says — POS, CIGAR, SEQ, QUAL, the reverse flag, XT — in numpy.  SEQ and QUAL of a record are in reference
orientation already, so no base is complemented here, no edit track is walked and no slot is searched (the product does all three,
mapad_amd/csrc/panel_core.hpp).  Shared by tests/test_panel_host.py (records from the host path) and tests/test_gpu_panel.py (records from the device, BAM
files the CLI wrote)."""
import numpy as np

from mapad_amd import synth

import pileup_util as pu

SCALARS = ("reads_seen", "reads", "reads_on_panel", "columns_counted", "columns_not_acgt", "columns_masked", "columns_low_quality", "columns_deleted")
WORDS = ("rows", "rows_unplaced", "rows_bad_alleles", "rows_transition", "rows_covered", "rows_called", "called_ref", "called_alt", "transitions_called", "obs_ref",
         "obs_alt", "obs_other", "max_depth")
SPLIT = 250_007            # the world of tests/test_gpu_pileup.py: 400 kbp in two contigs, the repeat at 300 000
LENGTHS = [SPLIT, 400_000 - SPLIT]
DENSE_START, DENSE_LEN = 16_300, 200  # every position of this stretch of c1 is a row: a 150-base read inside it spans more than 64 slots
PAIRS_AT = (1_003, 2_003, 3_003, 4_003, 5_003)  # positions of c1 that carry two rows with different alleles
DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
_M64 = (1 << 64) - 1


def world_genome():
    g = synth.genome(400_000, seed=77)
    g[300_000:300_400] = g[100_000:100_400]
    return g


def _next(b, k=1):
    """uint8 bases -> the k-th next base in ACGT: A -> C -> G -> T -> A"""
    return pu.LETTERS[(pu._CODE[b] + k) & 3]


def panel(g, seed=11):
    """The test panel over the world, rows in shuffled order -> {"tid", "pos0", "ref", "alt": one entry per row, "planted": the rows on the planted-variant sites
    of pileup_util.planted (their alt is the planted base), "rows_at": {absolute position: [rows]}}.  Every 97th position with alt = the next base in ACGT (all
    transversions) and every 101st with alt = the next but one (all transitions), so that both kinds mix; every position of the dense stretch; the first and
    last base of each contig; the planted sites; five positions with two rows of different alleles; unplaced rows (tid -1, tid past the last contig, pos0 == the
    contig's length); rows with alleles N/A, A/A and lower case."""
    rows = []  # (tid, pos0, ref, alt)

    def at(x, alt, ref=None):
        tid = 0 if x < SPLIT else 1
        rows.append((tid, x - (SPLIT if tid else 0), int(g[x]) if ref is None else ref, int(alt)))

    for x in range(0, 400_000, 97):
        at(x, _next(g[x]))
    for x in range(50, 400_000, 101):
        at(x, _next(g[x], 2))
    for x in range(DENSE_START, DENSE_START + DENSE_LEN):
        at(x, _next(g[x], 1 + (x & 1)))
    for x in (0, SPLIT - 1, SPLIT, 400_000 - 1):
        at(x, _next(g[x], 2))
    copy, sites, _ = pu.planted(g)
    first_planted = len(rows)
    for k in sites:
        at(pu.PLANT_START + int(k), copy[k])
    planted_rows = list(range(first_planted, len(rows)))
    for x in PAIRS_AT:
        at(x, _next(g[x], 1))
        at(x, _next(g[x], 3))
    rows += [(-1, 10, ord("A"), ord("C")), (2, 10, ord("A"), ord("C")), (0, SPLIT, ord("A"), ord("C")), (1, LENGTHS[1], ord("G"), ord("T")), (7, 0, ord("C"), ord("T"))]
    for x, ref, alt in ((7_001, "N", "A"), (7_002, "A", "A"), (7_003, "A", "n"), (7_004, "-", "C")):
        at(x, ord(alt), ord(ref))
    for x in (8_001, 8_002, 8_003):  # lower case is as good as upper case
        at(x, ord(chr(_next(g[x], 2)).lower()), ord(chr(g[x]).lower()))
    order = np.random.default_rng(seed).permutation(len(rows))
    where = np.empty(len(rows), np.int64)
    where[order] = np.arange(len(rows))
    rows = [rows[i] for i in order]
    p = {"tid": np.array([r[0] for r in rows], np.int32), "pos0": np.array([r[1] for r in rows], np.uint64), "ref": np.array([r[2] for r in rows], np.uint8),
         "alt": np.array([r[3] for r in rows], np.uint8), "planted": where[planted_rows]}
    return p


def args(p):
    return p["tid"], p["pos0"], p["ref"], p["alt"]


def placed(lengths, p):
    tid, pos0 = p["tid"].astype(np.int64), p["pos0"].astype(np.int64)
    ok = (tid >= 0) & (tid < len(lengths))
    lens = np.array(lengths, np.int64)[np.where(ok, tid, 0)]
    return ok & (pos0 < lens)


def mixed_batch(g, n, seed):
    """reads of 20..150 bases with indels, reads from the repeat, and by hand: reads on the contigs' first and last bases, 150-base reads inside the dense stretch on
    either strand (more than 64 slots each), reads with a deletion inside the dense stretch on either strand, a read with an N on a row, a read between rows"""
    d = DENSE_START
    hand = pu.hand_made([g[0:40], g[SPLIT:SPLIT + 40], g[SPLIT - 40:SPLIT], g[400_000 - 40:400_000], synth.revcomp(g[SPLIT - 45:SPLIT]),
                         g[d + 10:d + 160], synth.revcomp(g[d + 30:d + 180]),
                         np.concatenate([g[d + 20:d + 50], g[d + 52:d + 80]]), synth.revcomp(np.concatenate([g[d + 100:d + 130], g[d + 132:d + 160]])),
                         _with(g[d + 40:d + 90], 20, ord("N")), g[98:140]])
    return pu.concat(synth.reads(g, n, seed=seed, qual_range=(20, 40), damage=DMG, len_range=(20, 150), indel_frac=0.3),
                     synth.reads(g[100_000:100_400], n // 10, 45, seed=seed + 1, exo_frac=0.0, damage=DMG), hand)


def _with(read, at, b):
    read = read.copy()
    read[at] = b
    return read


def table(lengths, records, p, mode, min_bq=0, mask5=0, mask3=0):
    """records: the rows pileup_util.table takes -> {"counts": int64[n_rows, 2, 4] (strand, base), the scalars}"""
    ok = placed(lengths, p)
    site = [np.zeros(n, bool) for n in lengths]
    cells = [np.zeros((n, 2, 4), np.int64) for n in lengths]
    for t, x in zip(p["tid"][ok], p["pos0"][ok]):
        site[int(t)][int(x)] = True
    s = {k: 0 for k in SCALARS}
    for mapped, tid, pos, cigar, seq, qual, reverse, xt in records:
        s["reads_seen"] += 1
        if not mapped or (mode == 2 and xt != "U"):
            continue
        s["reads"] += 1
        ops = [(int(n), op) for n, op in pu._CIGAR.findall(cigar)]
        span = sum(n for n, op in ops if op != "I")
        if not site[tid][pos:pos + span].any():
            continue
        s["reads_on_panel"] += 1
        L = len(seq)
        i, x = 0, pos  # position in SEQ, position on the contig
        for n, op in ops:
            if op == "I":
                i += n
            elif op == "D":
                s["columns_deleted"] += int(site[tid][x:x + n].sum())
                x += n
            else:
                on = np.flatnonzero(site[tid][x:x + n])
                at = i + on
                given = L - 1 - at if reverse else at
                base = pu._CODE[seq[at]]
                acgt = base < 4
                masked = acgt & ((given < mask5) | (L - 1 - given < mask3))
                low = acgt & ~masked & (qual[at].astype(np.int64) < min_bq)
                keep = acgt & ~masked & ~low
                s["columns_not_acgt"] += int((~acgt).sum())
                s["columns_masked"] += int(masked.sum())
                s["columns_low_quality"] += int(low.sum())
                s["columns_counted"] += int(keep.sum())
                np.add.at(cells[tid], (x + on[keep], int(bool(reverse)), base[keep]), 1)
                i += n
                x += n
    counts = np.zeros((len(ok), 2, 4), np.int64)
    for r in np.flatnonzero(ok):
        counts[r] = cells[int(p["tid"][r])][int(p["pos0"][r])]
    s["counts"] = counts
    return s


def from_records(lengths, recs, batch, p, mode, min_bq=0, mask5=0, mask3=0):
    return table(lengths, pu.record_rows(recs, *batch), p, mode, min_bq, mask5, mask3)


def from_bam(lengths, bam_records, p, mode, min_bq=0, mask5=0, mask3=0):
    rows = []
    for r in bam_records:
        mapped = not r["flags"] & 0x4
        rows.append((mapped, r["tid"], r["pos"], r["cigar"], np.frombuffer(r["seq"].encode(), np.uint8), np.frombuffer(r["qual"].encode(), np.uint8) - 33,
                     bool(r["flags"] & 0x10), r["tags"]["XT"][1] if mapped else None))
    return table(lengths, rows, p, mode, min_bq, mask5, mask3)


def mix(seed, i):
    """the draw's 64 bits for row i, in np.uint64 arithmetic"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & _M64) + np.uint64(i + 1) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return int(z ^ (z >> np.uint64(31)))


def used_strands(r, a, transitions):
    """allele codes of a valid row -> the strands its call looks at"""
    if transitions == 2 and {r, a} == {1, 3}:
        return (1,)  # C/T: reverse-strand reads only
    if transitions == 2 and {r, a} == {0, 2}:
        return (0,)  # G/A: forward-strand reads only
    return (0, 1)


def calls(lengths, p, counts, call=0, min_depth=1, transitions=0, seed=0):
    """-> (uint8[n_rows] of '2' / '0' / '9', the summary words, per row (n_ref, n) or None where the row is not observed at all)"""
    ok = placed(lengths, p)
    w = {k: 0 for k in WORDS}
    out = np.full(len(ok), ord("9"), np.uint8)
    seen = [None] * len(ok)
    for i in range(len(ok)):
        w["rows"] += 1
        r, a = int(pu._CODE[p["ref"][i]]), int(pu._CODE[p["alt"][i]])
        valid = r < 4 and a < 4 and r != a
        if not ok[i]:
            w["rows_unplaced"] += 1
            continue
        if not valid:
            w["rows_bad_alleles"] += 1
            continue
        transition = {r, a} in ({1, 3}, {0, 2})
        w["rows_transition"] += transition
        c = sum(counts[i][s] for s in used_strands(r, a, transitions))
        n_ref, n_alt, total = int(c[r]), int(c[a]), int(c.sum())
        n = n_ref + n_alt
        w["rows_covered"] += total >= 1
        w["obs_ref"] += n_ref
        w["obs_alt"] += n_alt
        w["obs_other"] += total - n
        w["max_depth"] = max(w["max_depth"], total)
        seen[i] = (n_ref, n)
        if (transition and transitions == 1) or n < min_depth:
            continue
        is_ref = ((mix(seed, i) * n) >> 64) < n_ref
        if call == 1 and n_ref != n_alt:
            is_ref = n_ref > n_alt
        out[i] = ord("2") if is_ref else ord("0")
        w["rows_called"] += 1
        w["called_ref"] += is_ref
        w["called_alt"] += not is_ref
        w["transitions_called"] += transition
    return out, {k: int(v) for k, v in w.items()}, seen


RULES = [dict(call=0, min_depth=1, transitions=0, seed=0), dict(call=1, min_depth=2, transitions=1, seed=5), dict(call=0, min_depth=1, transitions=2, seed=(1 << 64) - 3),
         dict(call=1, min_depth=1, transitions=2, seed=12345)]


def assert_equal(acc_summary, acc_counts, acc_calls, want, lengths, p, what="", rules=RULES):
    """acc_summary(rule) / acc_counts(row_from, n) / acc_calls(row_from, n, rule): a Context's or a SnpPanelHost's read-outs; want: a table of this module"""
    n_rows = len(p["tid"])
    got_counts = acc_counts(0, n_rows).astype(np.int64)
    assert np.array_equal(got_counts, want["counts"]), (what, "counts", np.flatnonzero((got_counts != want["counts"]).any(axis=(1, 2)))[:10])
    assert np.array_equal(acc_counts(n_rows // 3, 100).astype(np.int64), want["counts"][n_rows // 3:n_rows // 3 + 100]), (what, "a window of counts")
    for rule in rules:
        got = acc_summary(rule)
        for k in SCALARS:
            assert got[k] == want[k], (what, k, got[k], want[k])
        c, w, _ = calls(lengths, p, want["counts"], **rule)
        for k in WORDS:
            assert got[k] == w[k], (what, rule, k, got[k], w[k])
        assert got["rule"] == {k: int(v) for k, v in rule.items()} and got["n_rows"] == n_rows, (what, rule)
        assert np.array_equal(acc_calls(0, n_rows, rule), c), (what, rule, "calls", np.flatnonzero(acc_calls(0, n_rows, rule) != c)[:10])
        assert np.array_equal(acc_calls(n_rows - 77, 77, rule), c[-77:]), (what, rule, "a window of calls")  # a call is its row's, wherever the window starts
        assert got["rows_called"] == got["called_ref"] + got["called_alt"] == int((c != ord("9")).sum()), (what, rule)
