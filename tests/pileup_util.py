"""The pileup computed independently of the product: A/C/G/T counts per reference position, the skip counters, the calls and the per-contig statistics from
what a BAM record says — POS, CIGAR, SEQ, QUAL, the reverse flag, XT — in numpy.  SEQ and QUAL of a record are in reference orientation already, so no base is
complemented here and no edit track is walked (the product does both, mapad_amd/csrc/pileup_core.hpp); only the end masks have to go back to positions of the
read as it was given.  Shared by tests/test_pileup_host.py (records from the host path) and tests/test_gpu_pileup.py (records from the device, BAM files the
CLI wrote)."""
import re

import numpy as np

from coverage_util import concat, hand_made  # noqa: F401  (batches are built the same way)

_CIGAR = re.compile(r"(\d+)([MID])")
_CODE = np.full(256, 4, np.int64)
for _k, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _k
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip("ACGTacgt", "TGCAtgca"):
    _COMP[ord(_a)] = ord(_b)
LETTERS = np.frombuffer(b"ACGTN", np.uint8)
SCALARS = ("reads", "reads_seen", "columns_counted", "columns_not_acgt", "columns_masked", "columns_low_quality", "deleted_columns", "insertions")


def table(lengths, records, mode, min_bq=0, mask5=0, mask3=0):
    """lengths: contig lengths in index order; records: (mapped, tid, pos (0-based), cigar, seq (uint8, reference orientation), qual (uint8, raw Phred, reference
    orientation), reverse, xt) each -> {"counts": [int64[n, 4] per contig], the scalars}"""
    counts = [np.zeros((n, 4), np.int64) for n in lengths]
    t = {k: 0 for k in SCALARS}
    for mapped, tid, pos, cigar, seq, qual, reverse, xt in records:
        t["reads_seen"] += 1
        if not mapped or (mode == 2 and xt != "U"):
            continue
        t["reads"] += 1
        L = len(seq)
        i, p = 0, pos  # position in SEQ, position on the contig
        for n, op in _CIGAR.findall(cigar):
            n = int(n)
            if op == "I":
                t["insertions"] += n
                i += n
            elif op == "D":
                t["deleted_columns"] += n
                p += n
            else:
                at = np.arange(i, i + n)
                given = L - 1 - at if reverse else at  # the position of SEQ[at] in the read as it was given
                base = _CODE[seq[at]]
                acgt = base < 4
                masked = acgt & ((given < mask5) | (L - 1 - given < mask3))
                low = acgt & ~masked & (qual[at].astype(np.int64) < min_bq)
                keep = acgt & ~masked & ~low
                t["columns_not_acgt"] += int((~acgt).sum())
                t["columns_masked"] += int(masked.sum())
                t["columns_low_quality"] += int(low.sum())
                t["columns_counted"] += int(keep.sum())
                np.add.at(counts[tid], (p + np.flatnonzero(keep), base[keep]), 1)
                i += n
                p += n
        assert i == L and p <= lengths[tid], (tid, pos, cigar, L)
    t["counts"] = counts
    return t


def calls(counts, min_depth, min_percent):
    """int64[n, 4] -> int64[n]: 0..3 = A, C, G, T, 4 = N — the call rule in integers"""
    d = counts.sum(axis=1)
    best = counts.max(axis=1)
    unique = (counts == best[:, None]).sum(axis=1) == 1
    ok = (d >= min_depth) & (best * 100 >= min_percent * d) & unique
    return np.where(ok, counts.argmax(axis=1), 4)


def consensus(counts, min_depth, min_percent):
    """-> uint8[n]: ord of 'A', 'C', 'G', 'T' or 'N'"""
    return LETTERS[calls(counts, min_depth, min_percent)]


def contig_stats(counts, min_depth, min_percent):
    d = counts.sum(axis=1)
    c = calls(counts, min_depth, min_percent)
    return {"length": int(len(d)), "sites_covered": int((d >= 1).sum()), "sites_deep": int((d >= min_depth).sum()), "sites_called": int((c < 4).sum()),
            "called": [int((c == b).sum()) for b in range(4)], "base_sum": [int(x) for x in counts.sum(axis=0)], "max_depth": int(d.max()) if len(d) else 0}


def record_rows(recs, seqs, quals, offsets):
    """recs: the list of dicts of mapad_amd.hits_to_records / Context.hits_to_records, and the reads they are of -> the rows table() takes.  SEQ / QUAL as the
    BAM record would hold them: the reverse complement / the reverse of a read reported on the reverse strand."""
    rows = []
    for r, rec in enumerate(recs):
        s, q = seqs[int(offsets[r]):int(offsets[r + 1])], quals[int(offsets[r]):int(offsets[r + 1])]
        if rec["reverse"]:
            s, q = _COMP[s[::-1]], q[::-1]
        rows.append((rec["mapped"], rec["tid"], rec["pos"], rec["cigar"], s, q, rec["reverse"], rec["xt"]))
    return rows


def from_records(lengths, recs, batch, mode, min_bq=0, mask5=0, mask3=0):
    return table(lengths, record_rows(recs, *batch), mode, min_bq, mask5, mask3)


def from_bam(lengths, bam_records, mode, min_bq=0, mask5=0, mask3=0):
    """bam_records: the third value of bam_util.read_bam"""
    rows = []
    for r in bam_records:
        mapped = not r["flags"] & 0x4
        rows.append((mapped, r["tid"], r["pos"], r["cigar"], np.frombuffer(r["seq"].encode(), np.uint8), np.frombuffer(r["qual"].encode(), np.uint8) - 33,
                     bool(r["flags"] & 0x10), r["tags"]["XT"][1] if mapped else None))
    return table(lengths, rows, mode, min_bq, mask5, mask3)


def assert_equal(got, want, min_depth, min_percent, what="", counts_of=None, consensus_of=None):
    """got: the dict of Context.pileup(min_depth, min_percent) / PileupHost.summary(...); want: a table of this module, or another such dict (then only the
    summaries are compared).  counts_of(tid, start, n) / consensus_of(tid, start, n, min_depth, min_percent): the window accessors of `got`'s source — every
    contig is then compared cell by cell and call by call with the table."""
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    if "counts" not in want:
        assert got["contigs"] == want["contigs"], what
        return
    assert got["min_depth"] == min_depth and got["min_percent"] == min_percent, what
    assert len(got["contigs"]) == len(want["counts"]), what
    for t, c in enumerate(want["counts"]):
        w = contig_stats(c, min_depth, min_percent)
        for k, v in w.items():
            assert got["contigs"][t][k] == v, (what, t, k, got["contigs"][t][k], v)
        if counts_of is not None:
            assert np.array_equal(counts_of(t, 0, len(c)).astype(np.int64), c), (what, "counts of contig", t)
        if consensus_of is not None:
            assert np.array_equal(consensus_of(t, 0, len(c), min_depth, min_percent), consensus(c, min_depth, min_percent)), (what, "consensus of contig", t)
    assert sum(sum(c["base_sum"]) for c in got["contigs"]) == got["columns_counted"], what


# ---- planted variants: a stretch of the genome copied with one base in 997 changed, and reads drawn from the copy -----------------------------------
PLANT_START, PLANT_LEN, PLANT_EVERY = 150_000, 20_000, 997


def planted(g, seed=5):
    """-> (the copy of g[PLANT_START : PLANT_START + PLANT_LEN] with every PLANT_EVERY-th base changed, the positions changed (within the stretch), a batch of
    4000 undamaged 50-base reads without indels drawn from the copy: 10x coverage)"""
    from mapad_amd import synth
    copy = g[PLANT_START:PLANT_START + PLANT_LEN].copy()
    at = np.arange(PLANT_EVERY // 2, PLANT_LEN, PLANT_EVERY)
    copy[at] = LETTERS[(_CODE[copy[at]] + 1) & 3]  # A -> C -> G -> T -> A
    return copy, at, synth.reads(copy, 4000, 50, seed=seed, subst_rate=0.01, exo_frac=0.0, qual_range=(20, 40), damage=None)


def assert_planted(copy, at, cons, reference):
    """cons: the consensus (min_depth 3, min_percent 80) over the stretch: every called position shows the copy's base — so the new base at every planted site
    that is called — and at least 90 % of the stretch is called"""
    called = cons != ord("N")
    assert np.array_equal(cons[called], copy[called]), np.flatnonzero(called & (cons != copy))[:10]
    assert int(called.sum()) * 10 >= 9 * len(copy), int(called.sum())
    assert called[at].sum() * 10 >= 9 * len(at) and (copy[at] != reference[at]).all() and np.array_equal(cons[at][called[at]], copy[at][called[at]])
