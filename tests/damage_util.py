"""The damage profile computed independently of the product: from what a BAM record says (CIGAR, MD, strand, XT) and the read, in numpy / plain Python.
Shared by tests/test_damage_host.py (records from the host path) and tests/test_gpu_damage.py (records from the device, BAM files the CLI wrote)."""
import re

import numpy as np

P = 32
_IDX = {"A": 0, "C": 1, "G": 2, "T": 3}
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")
_CIGAR = re.compile(r"(\d+)([MID])")
_MD = re.compile(r"(\d+)|\^([A-Za-z]+)|([A-Za-z])")


def take(batch, idx):
    """the reads idx (in that order) of a batch (seqs, quals, offsets) -> a new batch"""
    seqs, quals, offsets = batch
    off = offsets.astype(np.int64)
    lens = (off[1:] - off[:-1])[idx]
    new_off = np.zeros(len(idx) + 1, np.uint64)
    new_off[1:] = np.cumsum(lens)
    first = np.cumsum(lens) - lens
    src = np.repeat(off[:-1][idx] - first, lens) + np.arange(int(lens.sum()), dtype=np.int64)
    return seqs[src], quals[src], new_off


def with_duplicates(batch, n_copies, seed):
    """the batch plus n_copies reads drawn from it again, shuffled"""
    n = len(batch[2]) - 1
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = np.concatenate([np.arange(n), rng.integers(0, n, n_copies)])
    return take(batch, rng.permutation(idx))


def empty():
    return {"counts": np.zeros((2, P, 4, 4), np.uint64), "reads": 0, "reads_seen": 0, "aligned_bases": 0, "skipped_bases": 0, "insertions": 0, "deletions": 0}


def add_record(t, read, mapped, reverse, cigar, md, xt, mode):
    """read: the read as it was given to the mapper, 5' -> 3' (str); cigar / md / reverse as in the record (reference orientation)."""
    t["reads_seen"] += 1
    if not mapped or (mode == 2 and xt != "U"):
        return
    t["reads"] += 1
    L = len(read)
    seq = read.translate(_COMP)[::-1] if reverse else read  # SEQ of the record: reference orientation
    # MD -> the reference base of every aligned column (None: equal to the read's), deletions dropped
    ref_of = []
    for num, dele, mm in _MD.findall(md):
        if num:
            ref_of += [None] * int(num)
        elif mm:
            ref_of.append(mm)
    i = k = 0  # position in seq; aligned column
    for n, op in _CIGAR.findall(cigar):
        n = int(n)
        if op == "I":
            t["insertions"] += n
            i += n
        elif op == "D":
            t["deletions"] += n
        else:
            for _ in range(n):
                q = seq[i].upper()
                r = q if ref_of[k] is None else ref_of[k].upper()
                p = i
                if reverse:  # back into read orientation
                    q, r, p = q.translate(_COMP), r.translate(_COMP), L - 1 - i
                if q in _IDX and r in _IDX:
                    t["aligned_bases"] += 1
                    if p < P:
                        t["counts"][0, p, _IDX[r], _IDX[q]] += 1
                    if L - 1 - p < P:
                        t["counts"][1, L - 1 - p, _IDX[r], _IDX[q]] += 1
                else:
                    t["skipped_bases"] += 1
                i += 1
                k += 1
    assert i == L and k == len(ref_of), (cigar, md, L)


def from_records(recs, seqs, offsets, mode):
    """recs: the list of dicts of mapad_amd.hits_to_records / Context.hits_to_records"""
    t = empty()
    for r, rec in enumerate(recs):
        read = seqs[int(offsets[r]):int(offsets[r + 1])].tobytes().decode()
        add_record(t, read, rec["mapped"], rec["reverse"], rec["cigar"], rec["md"], rec["xt"], mode)
    return t


def from_bam(bam_records, mode):
    """bam_records: the third value of bam_util.read_bam.  SEQ of a reverse-strand record is the reverse complement of the read."""
    t = empty()
    for r in bam_records:
        mapped, reverse = not r["flags"] & 0x4, bool(r["flags"] & 0x10)
        read = r["seq"].translate(_COMP)[::-1] if reverse else r["seq"]
        add_record(t, read, mapped, reverse, r["cigar"], r["tags"]["MD"][1] if mapped else "", r["tags"]["XT"][1] if mapped else None, mode)
    return t


def assert_equal(got, want, what=""):
    """every counter both sides have (the 2048 cells and the scalars)"""
    for k in ("reads", "reads_seen", "aligned_bases", "skipped_bases", "insertions", "deletions"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(np.asarray(got["counts"], np.uint64), np.asarray(want["counts"], np.uint64)), what


def freq(counts, end, pos, ref, read):
    """e.g. freq(c, 0, 0, "C", "T"): C>T / (C>A + C>C + C>G + C>T) at 5' position 1"""
    row = counts[end, pos, _IDX[ref]].astype(np.float64)
    return float(row[_IDX[read]] / row.sum()) if row.sum() else 0.0
