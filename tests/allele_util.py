"""The allele likelihoods computed independently of the product's accumulation: per reference position the four int log-likelihood sums and the depth, the
skip counters, the calls, their qualities and the per-contig statistics from what a BAM record says — POS, CIGAR, SEQ, QUAL, the reverse flag, XT — in numpy,
with the per-column values taken row by row from mapad_allele_quantized_row (so nothing here knows the damage model).  SEQ and QUAL of a record are in
reference orientation; the table's rows are in read orientation, so a reverse record's base is complemented back for the lookup and its row is reversed
(allele a on the forward strand is true base 3 - a of the read).  Shared by tests/test_allele_host.py and tests/test_gpu_allele.py."""
import numpy as np

import mapad_amd
from pileup_util import _CIGAR, _CODE, LETTERS, SCALARS, concat, hand_made, record_rows  # noqa: F401

CONTIG_KEYS = ("length", "sites_covered", "sites_deep", "sites_called", "called", "max_depth", "margin_sum_q")


def min_margin_q(bits):
    """max(1, (int32)ceilf(bits * 256)) in float32, as the library computes it"""
    return max(1, int(np.ceil(np.float32(bits) * np.float32(256.0))))


class Rows:
    """mapad_allele_quantized_row, remembered per (read length, position, quality, read base)"""

    def __init__(self, params):
        self.params, self.seen = params, {}

    def __call__(self, L, p, q, to):
        k = (L, p, q, to)
        r = self.seen.get(k)
        if r is None:
            r = self.seen[k] = mapad_amd.allele_quantized_row(self.params, L, p, q, to).astype(np.int64)
        return r


def table(params, lengths, records, mode, min_bq=0, mask5=0, mask3=0, rows=None):
    """lengths: contig lengths in index order; records: the rows of pileup_util.record_rows -> {"ll": [int64[n, 4] per contig], "depth": [int64[n] per contig],
    the scalars}"""
    rows = rows or Rows(params)
    ll = [np.zeros((n, 4), np.int64) for n in lengths]
    depth = [np.zeros(n, np.int64) for n in lengths]
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
                for k in range(n):
                    at = i + k
                    given = L - 1 - at if reverse else at  # the position of SEQ[at] in the read as it was given
                    base = int(_CODE[seq[at]])
                    if base > 3:
                        t["columns_not_acgt"] += 1
                    elif given < mask5 or L - 1 - given < mask3:
                        t["columns_masked"] += 1
                    elif int(qual[at]) < min_bq:
                        t["columns_low_quality"] += 1
                    else:
                        t["columns_counted"] += 1
                        row = rows(L, given, int(qual[at]), 3 - base if reverse else base)
                        ll[tid][p + k] += row[::-1] if reverse else row
                        depth[tid][p + k] += 1
                i += n
                p += n
        assert i == L and p <= lengths[tid], (tid, pos, cigar, L)
    t["ll"], t["depth"] = ll, depth
    return t


def from_records(params, lengths, recs, batch, mode, min_bq=0, mask5=0, mask3=0, rows=None, skip=None):
    rr = record_rows(recs, *batch)
    if skip is not None:  # a skipped read is seen and nothing else: as if it were unmapped
        rr = [(False,) + r[1:] if skip[k] else r for k, r in enumerate(rr)]
    return table(params, lengths, rr, mode, min_bq, mask5, mask3, rows)


def calls(ll, depth, min_depth, margin_q):
    """int64[n, 4], int64[n] -> (int64[n] calls: 0..3 = A, C, G, T, 4 = N; int64[n] margins; int64[n] qualities) — the call rule in integers"""
    s = np.sort(ll, axis=1)
    margin = s[:, 3] - s[:, 2]
    ok = (depth >= min_depth) & (margin >= margin_q)
    call = np.where(ok, ll.argmax(axis=1), 4)
    return call, margin, np.where(ok, np.minimum(margin >> 8, 255), 0)


def consensus(ll, depth, min_depth, min_margin):
    """-> (uint8[n] ord of 'A', 'C', 'G', 'T' or 'N', uint8[n] qualities)"""
    c, _, q = calls(ll, depth, min_depth, min_margin_q(min_margin))
    return LETTERS[c], q.astype(np.uint8)


def contig_stats(ll, depth, min_depth, min_margin):
    c, m, _ = calls(ll, depth, min_depth, min_margin_q(min_margin))
    return {"length": int(len(depth)), "sites_covered": int((depth >= 1).sum()), "sites_deep": int((depth >= min_depth).sum()), "sites_called": int((c < 4).sum()),
            "called": [int((c == b).sum()) for b in range(4)], "max_depth": int(depth.max()) if len(depth) else 0, "margin_sum_q": int(m[c < 4].sum())}


def assert_equal(got, want, min_depth, min_margin, what="", cells_of=None, consensus_of=None):
    """got: the dict of Context.allele_summary(min_depth, min_margin) / AlleleHost.summary(...); want: a table of this module, or another such dict (then only the
    summaries are compared).  cells_of(tid, start, n) / consensus_of(tid, start, n, min_depth, min_margin): the window accessors of `got`'s source — every contig
    is then compared cell by cell and call by call with the table."""
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    if "ll" not in want:
        assert [{k: c[k] for k in CONTIG_KEYS} for c in got["contigs"]] == [{k: c[k] for k in CONTIG_KEYS} for c in want["contigs"]], what
        assert got["min_depth"] == want["min_depth"] and got["min_margin_q"] == want["min_margin_q"], what
        return
    assert got["min_depth"] == min_depth and got["min_margin_q"] == min_margin_q(min_margin), what
    assert len(got["contigs"]) == len(want["ll"]), what
    for t, (c, d) in enumerate(zip(want["ll"], want["depth"])):
        w = contig_stats(c, d, min_depth, min_margin)
        for k, v in w.items():
            assert got["contigs"][t][k] == v, (what, t, k, got["contigs"][t][k], v)
        if cells_of is not None:
            gl, gd = cells_of(t, 0, len(d))
            assert gl.dtype == np.int32 and gd.dtype == np.uint32
            assert np.array_equal(gd.astype(np.int64), d), (what, "depth of contig", t, np.flatnonzero(gd != d)[:10])
            assert np.array_equal(gl.astype(np.int64), c), (what, "cells of contig", t, np.argwhere(gl != c)[:10])
        if consensus_of is not None:
            gb, gq = consensus_of(t, 0, len(d), min_depth, min_margin)
            wb, wq = consensus(c, d, min_depth, min_margin)
            assert np.array_equal(gb, wb), (what, "consensus of contig", t, np.flatnonzero(gb != wb)[:10])
            assert np.array_equal(gq, wq), (what, "qualities of contig", t, np.flatnonzero(gq != wq)[:10])
    assert sum(int(d.sum()) for d in want["depth"]) == got["columns_counted"], what


def assert_same_accumulators(a, b, lengths, rules, what=""):
    """two sources with the accessors of AlleleHost (cells / consensus / summary): every cell, depth, call, quality and summary word equal"""
    for t, n in enumerate(lengths):
        (al, ad), (bl, bd) = a.cells(t, 0, n), b.cells(t, 0, n)
        assert np.array_equal(ad, bd), (what, "depth", t, np.flatnonzero(ad != bd)[:10])
        assert np.array_equal(al, bl), (what, "cells", t, np.argwhere(al != bl)[:10])
        for rule in rules:
            (ab, aq), (bb, bq) = a.consensus(t, 0, n, *rule), b.consensus(t, 0, n, *rule)
            assert np.array_equal(ab, bb) and np.array_equal(aq, bq), (what, "consensus", t, rule)
    for rule in rules:
        assert_equal(a.summary(*rule), b.summary(*rule), *rule, what=what)


class ContextView:
    """a Context under the accessor names of AlleleHost"""

    def __init__(self, ctx):
        self.cells, self.consensus, self.summary = ctx.allele_cells, ctx.allele_consensus, ctx.allele_summary
