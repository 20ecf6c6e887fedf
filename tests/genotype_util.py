"""The diploid genotype likelihoods computed independently of the product: the table row in numpy float64 from the f32 model values, the six heterozygous
cells per reference position from what a BAM record says (the walk of allele_util.table, with the per-column values row by row from
mapad_genotype_quantized_row), the call rule over the ten genotypes AA CC GG TT AC AG AT CG CT GT, GQ, PL and the per-contig statistics.  SEQ and QUAL of a
record are in reference orientation and the table's rows in read orientation: a reverse record's base is complemented back for the lookup and its row is taken
under the strand map (both alleles of a pair complemented: AC <-> GT, AG <-> CT; AT and CG stay).  Built on allele_util by import: the four homozygous cells,
the depth and the scalars are its table's.  Shared by tests/test_genotype_host.py and tests/test_gpu_genotype.py."""
import ctypes as C

import numpy as np

import mapad_amd
import allele_util as au
from pileup_util import _CIGAR, _CODE, record_rows

GENOTYPES = ("AA", "CC", "GG", "TT", "AC", "AG", "AT", "CG", "CT", "GT")
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
ALLELES = tuple((g, g) for g in range(4)) + PAIRS  # the two alleles of each of the ten genotypes
STRAND = np.array([5, 4, 2, 3, 1, 0])              # the read-orientation pair of a backward record's forward-strand pair
NO_CALL = 255
CONTIG_KEYS = au.CONTIG_KEYS


def penalty_q(bits):
    """(int32)ceilf(bits * 256) in float32, as the library computes it"""
    return int(np.ceil(np.float32(bits) * np.float32(256.0)))


def quantize(v):
    """float32 -> saturate_i16(rint(v * 256)), ties to even; a NaN lands on the lower end"""
    x = np.rint(np.float32(v) * np.float32(256.0))
    return -32768 if not x > -32768.0 else 32767 if x >= 32767.0 else int(x)


def model_values(params, length, pos, qual, to, nq):
    """the four f32 model values log2 P(to | x) for x = A, C, G, T, as tests/test_host_logic.py obtains sdm_get"""
    L = mapad_amd.lib()
    return [np.float32(L.mapad_sdm_get(C.byref(params), pos, length, ord("ACGT"[f]), ord("ACGT"[to]), qual if nq == 256 else 0)) for f in range(4)]


def restated_row(s):
    """s: the four f32 model values -> (int[6] pair values in 1/256 bit, bool[6]: the float64 value lies within 2^-12 of a rounding tie)"""
    out, near = [], []
    for x, y in PAIRS:
        with np.errstate(divide="ignore"):
            h = np.log2(0.5 * np.exp2(np.float64(s[x])) + 0.5 * np.exp2(np.float64(s[y])))
        out.append(quantize(np.float32(h)))
        u = float(h) * 256.0
        near.append(bool(np.isfinite(u) and abs(abs(u - np.floor(u)) - 0.5) < 2.0 ** -12))
    return out, near


class Rows:
    """mapad_genotype_quantized_row, remembered per (read length, position, quality, read base)"""

    def __init__(self, params):
        self.params, self.seen = params, {}

    def __call__(self, L, p, q, to):
        k = (L, p, q, to)
        r = self.seen.get(k)
        if r is None:
            r = self.seen[k] = mapad_amd.genotype_quantized_row(self.params, L, p, q, to).astype(np.int64)
        return r


def het_table(lengths, records, mode, min_bq=0, mask5=0, mask3=0, rows=None):
    """records: the rows of pileup_util.record_rows -> [int64[n, 6] per contig]: the walk of allele_util.table over the same columns"""
    het = [np.zeros((n, 6), np.int64) for n in lengths]
    for mapped, tid, pos, cigar, seq, qual, reverse, xt in records:
        if not mapped or (mode == 2 and xt != "U"):
            continue
        L = len(seq)
        i, p = 0, pos
        for n, op in _CIGAR.findall(cigar):
            n = int(n)
            if op == "I":
                i += n
            elif op == "D":
                p += n
            else:
                for k in range(n):
                    at = i + k
                    given = L - 1 - at if reverse else at
                    base = int(_CODE[seq[at]])
                    if base <= 3 and not (given < mask5 or L - 1 - given < mask3) and int(qual[at]) >= min_bq:
                        row = rows(L, given, int(qual[at]), 3 - base if reverse else base)
                        het[tid][p + k] += row[STRAND] if reverse else row
                i += n
                p += n
    return het


def from_records(params, lengths, recs, batch, mode, min_bq=0, mask5=0, mask3=0, rows=None, allele_rows=None, skip=None):
    """-> allele_util's table (ll, depth, scalars) with "het" beside them"""
    t = au.from_records(params, lengths, recs, batch, mode, min_bq, mask5, mask3, rows=allele_rows, skip=skip)
    rr = record_rows(recs, *batch)
    if skip is not None:
        rr = [(False,) + r[1:] if skip[k] else r for k, r in enumerate(rr)]
    t["het"] = het_table(lengths, rr, mode, min_bq, mask5, mask3, rows or Rows(params))
    return t


def values(ll, het, pen_q):
    """int64[n, 4], int64[n, 6] -> int64[n, 10]: what the rule compares"""
    return np.concatenate([np.asarray(ll, np.int64), np.asarray(het, np.int64) - int(pen_q)], axis=1)


def calls(ll, het, depth, min_depth, margin_q, pen_q):
    """-> (int64[n] genotype 0..9 or 255, int64[n] margins, int64[n] GQ, int64[n, 10] PL): the call rule in integers; argmax is the first maximum"""
    g = values(ll, het, pen_q)
    s = np.sort(g, axis=1)
    margin = s[:, 9] - s[:, 8]
    ok = (np.asarray(depth) >= min_depth) & (margin >= margin_q)
    call = np.where(ok, g.argmax(axis=1), NO_CALL)
    gq = np.where(ok, np.minimum(margin * 301 // 25600, 99), 0)
    pl = np.minimum((s[:, 9:10] - g) * 301 // 25600, 255)
    return call, margin, gq, pl


def contig_stats(ll, het, depth, min_depth, min_margin, het_penalty):
    c, m, _, _ = calls(ll, het, depth, min_depth, au.min_margin_q(min_margin), penalty_q(het_penalty))
    return {"length": int(len(depth)), "sites_covered": int((depth >= 1).sum()), "sites_deep": int((depth >= min_depth).sum()), "sites_called": int((c != NO_CALL).sum()),
            "called": [int((c == k).sum()) for k in range(10)], "max_depth": int(depth.max()) if len(depth) else 0, "margin_sum_q": int(m[c != NO_CALL].sum())}


def assert_equal(src, want, rule, what=""):
    """src: an object with genotype_summary / genotype_cells / genotype_calls (a Context or an AlleleHost); want: a table of from_records: every het cell,
    genotype byte, GQ byte and summary word under the rule (min_depth, min_margin, het_penalty)"""
    min_depth, min_margin, het_penalty = rule
    got = src.genotype_summary(*rule)
    assert got["on"] == 1 and got["min_depth"] == min_depth and got["min_margin_q"] == au.min_margin_q(min_margin) and got["het_penalty_q"] == penalty_q(het_penalty), (what, got)
    assert len(got["contigs"]) == len(want["het"]), what
    for t, (ll, het, d) in enumerate(zip(want["ll"], want["het"], want["depth"])):
        w = contig_stats(ll, het, d, *rule)
        for k, v in w.items():
            assert got["contigs"][t][k] == v, (what, t, k, got["contigs"][t][k], v)
        gh = src.genotype_cells(t, 0, len(d))
        assert gh.dtype == np.int32 and np.array_equal(gh.astype(np.int64), het), (what, "het cells of contig", t, np.argwhere(gh != het)[:10])
        gt, gq = src.genotype_calls(t, 0, len(d), *rule)
        wc, _, wq, _ = calls(ll, het, d, min_depth, au.min_margin_q(min_margin), penalty_q(het_penalty))
        assert gt.dtype == np.uint8 and np.array_equal(gt, wc), (what, "genotypes of contig", t, np.flatnonzero(gt != wc)[:10])
        assert np.array_equal(gq, wq), (what, "GQ of contig", t, np.flatnonzero(gq != wq)[:10])


def assert_same(a, b, lengths, rules, what=""):
    """two sources (Context / AlleleHost): every het cell, genotype, GQ and summary word equal"""
    for t, n in enumerate(lengths):
        ha, hb = a.genotype_cells(t, 0, n), b.genotype_cells(t, 0, n)
        assert np.array_equal(ha, hb), (what, "het cells", t, np.argwhere(ha != hb)[:10])
        for rule in rules:
            (ga, qa), (gb, qb) = a.genotype_calls(t, 0, n, *rule), b.genotype_calls(t, 0, n, *rule)
            assert np.array_equal(ga, gb) and np.array_equal(qa, qb), (what, "calls", t, rule, np.flatnonzero(ga != gb)[:10])
    for rule in rules:
        sa, sb = a.genotype_summary(*rule), b.genotype_summary(*rule)
        assert [{k: c[k] for k in CONTIG_KEYS} for c in sa["contigs"]] == [{k: c[k] for k in CONTIG_KEYS} for c in sb["contigs"]], (what, rule)
        assert all(sa[k] == sb[k] for k in ("on", "min_depth", "min_margin_q", "het_penalty_q", "batches")), (what, rule, sa, sb)


def second_haplotype(g, every, seed):
    """a copy of g with one substitution about every `every` bases -> (haplotype, positions)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    at = np.arange(every // 2, len(g) - every // 2, every) + rng.integers(-every // 4, every // 4 + 1, len(range(every // 2, len(g) - every // 2, every)))
    h = g.copy()
    code = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), g[at])
    h[at] = np.frombuffer(b"ACGT", np.uint8)[(code + rng.integers(1, 4, len(at))) & 3]
    return h, at
