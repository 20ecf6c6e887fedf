"""Quality rescaling computed independently of the product: the table from the models' formulas in numpy float64, and a read's rescaled qualities from what a
record says (CIGAR, MD, strand), the read and its qualities, in plain Python (tests/dscore_util.py is the pattern).  Shared by tests/test_rescale_host.py
(records from the host path) and tests/test_gpu_rescale.py (records from the device, BAM files the CLI wrote)."""
import numpy as np

from damage_util import _CIGAR, _COMP, _MD
from dscore_util import _VINDIJA

BINS = 64
CELLS = {("C", "T"): 0, ("G", "A"): 1}  # (reference base, read base) in read orientation
SCALARS = ("reads_seen", "reads_rescaled", "bases_changed", "quality_drop_sum")


def posterior_f64(p, L):
    """pd float64[L, 256, 2]: the posterior that a C->T (0) / G->A (1) mismatch at a read position and quality byte is damage, (P_dam - P_null) / P_dam clamped to
    [0, 1], from mapad_params_t `p`"""
    f32 = lambda x: float(np.float32(x))  # noqa: E731  (the parameters as the library holds them)
    i = np.arange(L, dtype=np.float64)[:, None]
    fp, tp = i + 1, (L - 1 - i) + 1
    p_dam, p_null = np.zeros((L, 256, 2)), np.zeros((L, 256, 2))
    if p.model_kind == 0:  # SimpleAncientDnaModel
        q = np.full((1, 256), 255.0) if p.ignore_base_quality else np.arange(256, dtype=np.float64)[None, :]
        seq_err = 10.0 ** (-q / 10.0) / 3.0
        div = f32(p.divergence)
        e = seq_err + div - seq_err * div
        f, t = f32(p.five_prime_overhang), f32(p.three_prime_overhang)
        if p.library_prep == 0:  # single-stranded: C->T from both ends, G->A at the double-stranded rate everywhere
            p_fwd, p_rev = f ** fp + t ** tp - f ** fp * t ** tp, np.zeros_like(fp)
        else:
            p_fwd, p_rev = f ** fp, f ** tp
        ss, ds = f32(p.ss_deamination_rate), f32(p.ds_deamination_rate)
        for cell, pr in ((0, p_fwd), (1, p_rev)):
            deam = ss * pr + ds * (1.0 - pr)
            p_dam[:, :, cell] = e + deam - 4.0 * e * deam
            p_null[:, :, cell] = e + 0.0 * deam
    elif p.model_kind == 1:  # VindijaPwm: the C row only
        k = np.minimum(np.arange(L), L - 1 - np.arange(L))
        ct = np.array([f32(_VINDIJA[x]) if x < 7 else f32(0.02) for x in k])
        sub = f32(0.0005)
        p_dam[:, :, 0], p_null[:, :, 0] = ct[:, None], sub
        p_dam[:, :, 1], p_null[:, :, 1] = sub, sub
    else:  # the test model: C->T scores deam_score instead of mm_score
        p_dam[:, :, 0], p_null[:, :, 0] = 2.0 ** f32(p.deam_score), 2.0 ** f32(p.mm_score)
        p_dam[:, :, 1], p_null[:, :, 1] = 2.0 ** f32(p.mm_score), 2.0 ** f32(p.mm_score)
    with np.errstate(divide="ignore", invalid="ignore"):
        pd = np.where(p_dam > 0.0, (p_dam - p_null) / p_dam, 0.0)
    return np.clip(pd, 0.0, 1.0)


def table_f64(p, L):
    """(q' before the floor as float64[L, 256, 2] — -10 log10(e') + 0.5, +inf where no logarithm is taken: pd == 0, e' >= 1, quality 255 —, the table uint8[L, 256, 2] the rule gives from it)"""
    pd = posterior_f64(p, L)
    q = np.arange(256, dtype=np.float64)[None, :, None]
    e = 10.0 ** (-q / 10.0)
    e2 = 1.0 - (1.0 - e) * (1.0 - pd)
    with np.errstate(divide="ignore"):
        raw = np.where((pd == 0.0) | (e2 <= 0.0), np.inf, -10.0 * np.log10(np.maximum(e2, 1e-300)) + 0.5)
    zero = (e2 >= 1.0) & (pd > 0.0)  # 0 by definition, no logarithm taken: never near anything
    raw = np.where(zero, np.inf, raw)
    tab = np.where(zero, 0.0, np.minimum(np.broadcast_to(q, raw.shape), np.maximum(np.floor(raw), 0.0)))
    tab[:, 255, :] = 255  # a missing quality stays missing
    raw[:, 255, :] = np.inf
    return raw, tab.astype(np.uint8)


def rescale_record(table, read, quals, mapped, reverse, cigar, md):
    """read / quals: as they were given to the mapper, 5' -> 3'; cigar / md / reverse as in the record (reference orientation); table: uint8[L, 256, 2].
    Returns (rescaled qualities uint8[L] in read orientation, candidate columns [C->T, G->A])."""
    out = np.array(quals, np.uint8)
    cols = [0, 0]
    if not mapped:
        return out, cols
    L = len(read)
    seq = read.translate(_COMP)[::-1] if reverse else read
    ref_of = []
    for num, dele, mm in _MD.findall(md):
        if num:
            ref_of += [None] * int(num)
        elif mm:
            ref_of.append(mm)
    i = k = 0
    for n, op in _CIGAR.findall(cigar):
        n = int(n)
        if op == "I":
            i += n
        elif op == "M":
            for _ in range(n):
                if ref_of[k] is not None:  # a mismatch
                    q, r, p = seq[i].upper(), ref_of[k].upper(), i
                    if reverse:  # back into read orientation
                        q, r, p = q.translate(_COMP), r.translate(_COMP), L - 1 - i
                    cell = CELLS.get((r, q))
                    if cell is not None:
                        cols[cell] += 1
                        if quals[p] != 255:
                            out[p] = table[p, int(quals[p]), cell]
                i += 1
                k += 1
    assert i == L and k == len(ref_of), (cigar, md, L)
    return out, cols


def from_records(params, recs, batch):
    """recs: the list of dicts of mapad_amd.hits_to_records / Context.hits_to_records -> (rescaled uint8 at the batch's offsets, summary)"""
    import mapad_amd
    seqs, quals, offsets = batch
    n = len(offsets) - 1
    tables = {}
    out = np.array(quals, np.uint8)
    s = {"reads_seen": n, "reads_rescaled": 0, "candidate_columns": np.zeros(2, np.uint64), "bases_changed": 0, "quality_drop_sum": 0, "new_quality": np.zeros(BINS, np.uint64)}
    for r, rec in enumerate(recs):
        a, b = int(offsets[r]), int(offsets[r + 1])
        if not rec["mapped"]:
            continue
        if b - a not in tables:
            tables[b - a] = mapad_amd.quality_rescale_table(params, b - a)
        nq, cols = rescale_record(tables[b - a], seqs[a:b].tobytes().decode(), quals[a:b], True, rec["reverse"], rec["cigar"], rec["md"])
        out[a:b] = nq
        s["reads_rescaled"] += 1
        s["candidate_columns"] += np.array(cols, np.uint64)
        ch = np.flatnonzero(nq != quals[a:b])
        s["bases_changed"] += len(ch)
        s["quality_drop_sum"] += int((quals[a:b][ch].astype(np.int64) - nq[ch].astype(np.int64)).sum())
        for v in nq[ch]:
            s["new_quality"][min(int(v), BINS - 1)] += 1
    return out, s


def assert_summary(got, want, what=""):
    """every counter both sides have"""
    for k in SCALARS:
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])
    for k in ("candidate_columns", "new_quality"):
        assert np.array_equal(np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64)), (what, k)
    if "batches" in got and "batches" in want:
        assert got["batches"] == want["batches"], (what, got["batches"], want["batches"])
