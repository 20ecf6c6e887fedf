"""Depth of coverage computed independently of the product: per-base depth per contig from what a record says (contig, position, CIGAR, XT), in numpy.
Shared by tests/test_coverage_host.py (records from the host path) and tests/test_gpu_coverage.py (records from the device, BAM files the CLI wrote)."""
import re

import numpy as np

BINS = 256
_CIGAR = re.compile(r"(\d+)([MID])")


def concat(*batches):
    """batches (seqs, quals, offsets) one behind the other"""
    seqs = np.concatenate([b[0] for b in batches])
    quals = np.concatenate([b[1] for b in batches])
    offs, base = [np.zeros(1, np.uint64)], 0
    for b in batches:
        offs.append(b[2][1:] + np.uint64(base))
        base += int(b[2][-1])
    return seqs, quals, np.concatenate(offs)


def hand_made(pieces, qual=30):
    """reads given as uint8 arrays -> a batch"""
    offs = np.zeros(len(pieces) + 1, np.uint64)
    offs[1:] = np.cumsum([len(p) for p in pieces])
    seqs = np.concatenate(pieces).astype(np.uint8)
    return seqs, np.full(len(seqs), qual, np.uint8), offs


def table(lengths, records, mode):
    """lengths: contig lengths in index order; records: (mapped, tid, pos (0-based), cigar, xt) each -> the table"""
    depth = [np.zeros(n, np.int64) for n in lengths]
    t = {"reads": 0, "reads_seen": 0, "covered_columns": 0, "deleted_columns": 0, "insertions": 0, "contig_reads": [0] * len(lengths)}
    for mapped, tid, pos, cigar, xt in records:
        t["reads_seen"] += 1
        if not mapped or (mode == 2 and xt != "U"):
            continue
        t["reads"] += 1
        t["contig_reads"][tid] += 1
        p = pos
        for n, op in _CIGAR.findall(cigar):
            n = int(n)
            if op == "M":
                depth[tid][p:p + n] += 1
                t["covered_columns"] += n
                p += n
            elif op == "D":
                t["deleted_columns"] += n
                p += n
            else:
                t["insertions"] += n
        assert p <= lengths[tid], (tid, pos, cigar)
    t["depth"] = depth
    t["contigs"] = [{"length": int(len(d)), "reads": t["contig_reads"][k], "covered_bases": int((d > 0).sum()), "depth_sum": int(d.sum()), "max_depth": int(d.max()) if len(d) else 0}
                    for k, d in enumerate(depth)]
    t["hist"] = np.bincount(np.minimum(np.concatenate(depth), BINS - 1), minlength=BINS).astype(np.uint64)
    return t


def from_records(lengths, recs, mode):
    """recs: the list of dicts of mapad_amd.hits_to_records / Context.hits_to_records"""
    return table(lengths, [(r["mapped"], r["tid"], r["pos"], r["cigar"], r["xt"]) for r in recs], mode)


def from_bam(lengths, bam_records, mode):
    """bam_records: the third value of bam_util.read_bam"""
    rows = []
    for r in bam_records:
        mapped = not r["flags"] & 0x4
        rows.append((mapped, r["tid"], r["pos"], r["cigar"], r["tags"]["XT"][1] if mapped else None))
    return table(lengths, rows, mode)


def assert_equal(got, want, what="", depth_of=None):
    """got: the dict of Context.coverage() / CoverageHost.summary(); want: a table of this module, or another such dict.  depth_of(tid, start, n): the window
    accessor of `got`'s source — every contig is then compared base by base with want["depth"]."""
    for k in ("reads", "reads_seen", "covered_columns", "deleted_columns", "insertions"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert len(got["contigs"]) == len(want["contigs"]), what
    for t, (g, w) in enumerate(zip(got["contigs"], want["contigs"])):
        for k in ("length", "reads", "covered_bases", "depth_sum", "max_depth"):
            assert g[k] == w[k], (what, t, k, g[k], w[k])
    assert np.array_equal(np.asarray(got["hist"], np.uint64), np.asarray(want["hist"], np.uint64)), what
    if depth_of is not None:
        for t, d in enumerate(want["depth"]):
            assert np.array_equal(depth_of(t, 0, len(d)).astype(np.int64), d), (what, "depth of contig", t)
