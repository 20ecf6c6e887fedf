"""PCR duplicates computed independently of the product: a grouping of the records, in conversion order, by what a BAM record says — contig, position, strand
and the sum of the M and D lengths of the CIGAR — where the first index wins.  It never looks at absolute text positions, the edit track or the table
(mapad_amd/csrc/dedup_core.hpp does).  Shared by tests/test_dedup_host.py (records from the host path) and tests/test_gpu_dedup.py (records from the device,
BAM files the CLI wrote)."""
import re

import numpy as np

BINS = 256
_CIGAR = re.compile(r"(\d+)([MID])")


def span(cigar):
    """reference bases an alignment covers: the M and D lengths"""
    return sum(int(n) for n, op in _CIGAR.findall(cigar) if op in "MD")


def key_of(mapped, tid, pos, reverse, cigar):
    return (int(tid), int(pos), bool(reverse), span(cigar)) if mapped else None


def grouping(keys):
    """keys: one per read in conversion order, None = not eligible -> (flags uint8[n], stats like Context.duplicates())"""
    first, members, flags = {}, {}, np.zeros(len(keys), np.uint8)
    for i, k in enumerate(keys):
        if k is None:
            continue
        if k in first:
            flags[i] = 1
        else:
            first[k] = i
        members[k] = members.get(k, 0) + 1
    hist = np.bincount(np.minimum(np.array(list(members.values()), np.int64), BINS - 1), minlength=BINS).astype(np.uint64) if members else np.zeros(BINS, np.uint64)
    stats = {"reads_seen": len(keys), "reads_eligible": sum(k is not None for k in keys), "duplicates": int(flags.sum()), "fragments": len(first), "histogram": hist}
    return flags, stats


def from_records(recs):
    """recs: the dicts of mapad_amd.hits_to_records / Context.hits_to_records, all batches one behind the other in conversion order"""
    return grouping([key_of(r["mapped"], r["tid"], r["pos"], r["reverse"], r["cigar"]) for r in recs])


def from_bam(bam_records):
    """bam_records: the third value of bam_util.read_bam"""
    return grouping([key_of(not r["flags"] & 0x4, r["tid"], r["pos"], bool(r["flags"] & 0x10), r["cigar"]) for r in bam_records])


def assert_stats(got, want, what=""):
    for k in ("reads_seen", "reads_eligible", "duplicates", "fragments"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(np.asarray(got["histogram"], np.uint64), np.asarray(want["histogram"], np.uint64)), what
    assert got["fragments"] == got["reads_eligible"] - got["duplicates"] == int(np.asarray(got["histogram"]).sum()), what


def masked(recs, flags):
    """the records with the flagged ones' `mapped` cleared: what the numpy tables of the three analyses are built from under mode 2"""
    return [dict(r, mapped=False) if f else r for r, f in zip(recs, flags)]
