"""The damage score computed independently of the product: the table from the models' formulas in numpy float64, and a read's score from what a record says
(CIGAR, MD, strand), the read and its qualities, in plain Python (tests/damage_util.py: add_record is the pattern).  Shared by tests/test_dscore_host.py
(records from the host path) and tests/test_gpu_dscore.py (records from the device, BAM files the CLI wrote)."""
import numpy as np

from damage_util import _CIGAR, _COMP, _MD

BINS = 128
CELLS = {("C", "C"): 0, ("C", "T"): 1, ("G", "G"): 2, ("G", "A"): 3}  # (reference base, read base) in read orientation
EPS = float(np.finfo(np.float32).eps)
_VINDIJA = [0.4, 0.25, 0.1, 0.06, 0.05, 0.04, 0.03]


def table_f64(p, L):
    """(delta in units of 1/256 bit as float64[L, nq, 4], before rounding) from mapad_params_t `p`: sdm_get - sdm_get_null for C->C, C->T, G->G, G->A"""
    f32 = lambda x: float(np.float32(x))  # noqa: E731  (the parameters as the library holds them)
    i = np.arange(L, dtype=np.float64)[:, None]
    fp, tp = i + 1, (L - 1 - i) + 1
    if p.model_kind == 0:  # SimpleAncientDnaModel
        nq = 1 if p.ignore_base_quality else 256
        q = np.full((1, 1), 255.0) if p.ignore_base_quality else np.arange(256, dtype=np.float64)[None, :]
        seq_err = 10.0 ** (-q / 10.0) / 3.0
        div = f32(p.divergence)
        e = seq_err + div - seq_err * div
        no_err = 1.0 - 3.0 * e
        f, t = f32(p.five_prime_overhang), f32(p.three_prime_overhang)
        if p.library_prep == 0:  # single-stranded: C->T from both ends, no G->A
            p_fwd, p_rev = f ** fp + t ** tp - f ** fp * t ** tp, np.zeros_like(fp)
        else:
            p_fwd, p_rev = f ** fp, f ** tp
        ss, ds = f32(p.ss_deamination_rate), f32(p.ds_deamination_rate)
        out = np.zeros((L, nq, 4))
        lg = lambda v: np.log2(np.maximum(v, EPS))  # noqa: E731
        for pr, same, other in ((p_fwd, 0, 1), (p_rev, 2, 3)):
            deam = ss * pr + ds * (1.0 - pr)
            out[:, :, same] = lg(no_err - deam + 4.0 * e * deam) - lg(no_err + 0.0 * deam)
            out[:, :, other] = lg(e + deam - 4.0 * e * deam) - lg(e + 0.0 * deam)
        return out * 256.0
    if p.model_kind == 1:  # VindijaPwm: the C row only
        k = np.minimum(np.arange(L), L - 1 - np.arange(L))
        ct = np.array([_VINDIJA[x] if x < 7 else 0.02 for x in k])
        sub = f32(0.0005)
        out = np.zeros((L, 1, 4))
        out[:, 0, 0] = np.log2(1.0 - ct) - np.log2(1.0 - sub)
        out[:, 0, 1] = np.log2(ct) - np.log2(sub)
        return out * 256.0
    out = np.zeros((L, 1, 4))  # the test model: C->T scores deam_score instead of mm_score
    out[:, 0, 1] = f32(p.deam_score) - f32(p.mm_score)
    return out * 256.0


def score_record(table, read, quals, mapped, reverse, cigar, md):
    """read / quals: as they were given to the mapper, 5' -> 3'; cigar / md / reverse as in the record (reference orientation); table: int16[L, nq, 4].
    Returns (score_q, scored, informative columns)."""
    if not mapped:
        return 0, 0, 0
    L, nq = len(read), table.shape[1]
    seq = read.translate(_COMP)[::-1] if reverse else read
    ref_of = []
    for num, dele, mm in _MD.findall(md):
        if num:
            ref_of += [None] * int(num)
        elif mm:
            ref_of.append(mm)
    i = k = 0
    score = cols = 0
    for n, op in _CIGAR.findall(cigar):
        n = int(n)
        if op == "I":
            i += n
        elif op == "M":
            for _ in range(n):
                q = seq[i].upper()
                r = q if ref_of[k] is None else ref_of[k].upper()
                p = i
                if reverse:  # back into read orientation
                    q, r, p = q.translate(_COMP), r.translate(_COMP), L - 1 - i
                cell = CELLS.get((r, q))
                if cell is not None:
                    score += int(table[p, int(quals[p]) if nq > 1 else 0, cell])
                    cols += 1
                i += 1
                k += 1
    assert i == L and k == len(ref_of), (cigar, md, L)
    return score, 1, cols


def from_records(params, recs, batch, threshold_q=0):
    """recs: the list of dicts of mapad_amd.hits_to_records / Context.hits_to_records -> (score_q int32[n], scored uint8[n], summary)"""
    import mapad_amd
    seqs, quals, offsets = batch
    n = len(offsets) - 1
    tables = {}
    score_q, scored = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    s = {"reads_seen": n, "reads_scored": 0, "reads_below": 0, "informative_columns": 0, "score_sum": 0, "histogram": np.zeros(BINS, np.uint64)}
    for r, rec in enumerate(recs):
        a, b = int(offsets[r]), int(offsets[r + 1])
        if rec["mapped"] and b - a not in tables:
            tables[b - a] = mapad_amd.damage_score_table(params, b - a)
        sq, sc, cols = score_record(tables.get(b - a), seqs[a:b].tobytes().decode(), quals[a:b], rec["mapped"], rec["reverse"], rec["cigar"], rec["md"])
        score_q[r], scored[r] = sq, sc
        if sc:
            s["reads_scored"] += 1
            s["reads_below"] += sq < threshold_q
            s["informative_columns"] += cols
            s["score_sum"] += sq
            s["histogram"][(min(max(sq, -8192), 8191) + 8192) >> 7] += 1
    return score_q, scored, s


def assert_summary(got, want, what=""):
    """every counter both sides have"""
    for k in ("reads_seen", "reads_scored", "reads_below", "informative_columns", "score_sum"):
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])
    assert np.array_equal(np.asarray(got["histogram"], np.uint64), np.asarray(want["histogram"], np.uint64)), what
    for k in ("batches", "threshold_q"):
        if k in got and k in want:
            assert got[k] == want[k], (what, k, got[k], want[k])
