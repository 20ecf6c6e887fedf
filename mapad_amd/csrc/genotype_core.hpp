// genotype_core.hpp — diploid genotype likelihoods per reference position, riding on the allele likelihoods (allele_core.hpp): the ten unordered pairs of
// forward-strand alleles, in the fixed order AA CC GG TT AC AG AT CG CT GT (0..9).  The four homozygous values of a position ARE the allele cells ll[S][4],
// and depth[S] is theirs; this file adds the six heterozygous cells int32 het[S][6] (AC AG AT CG CT GT, units of 1/256 bit, 24 bytes per position) and the
// call rule over all ten.  A heterozygous genotype's column likelihood is a log of a sum, so it does not decompose into per-allele sums: it gets its own table.
// One source for genotype_kernel, genotype_call_kernel (mapad_amd.hip), the host path (mapad_allele_host_* with genotypes on) and a stand-alone self-test
// (tests/emu/genotype_selftest.cpp).
//
// Definition.  Which reads and columns count is the allele accumulator's rule exactly (same mode, PileupFilter, skip array, pileup_column, coverage_ref_op
// walk), so ll, depth and het always describe the same columns.  For a counted column of read base `to` at read position p with quality level ql, with
// s_x = sdm_get(p, L, x, to, ql) (f32, log2 P(to | true base x)), the pair {x, y} in READ orientation is worth
//     h = log2(0.5 * 2^s_x + 0.5 * 2^s_y),
// evaluated on the host in double from the two f32 values, converted to f32 and rounded by host::dscore_quantize (host_models.hpp: genotype_table).  The table
// holds, per read length, int16 [len][nq][4 read bases][8]: the six pair values AC AG AT CG CT GT by `from` pair in read orientation, then two zero words — a
// row is one aligned 16-byte load.  The device never evaluates a transcendental: it loads the rounded row and adds integers,
//     het[abs + o][k] += row[backward ? genotype_strand_pair(k) : k]   for k = 0..5,
// where genotype_strand_pair complements both alleles: AC <-> GT, AG <-> CT, and AT and CG, their own complements, stay (5 - k for the four that move) — the
// het counterpart of allele_column_values' 3 - a.  Wrapping is two's complement; a cell can wrap only beyond 65 536 columns of depth (not checked).  Every index
// is checked against S before it is written; an alignment that leaves the text or a length without a table is reported, not written.
//
// Call rule, integers only, in int64.  g[0..3] = the ll cells, g[4..9] = the het cells - het_penalty_q (>= 0; applied at the call, never stored).  best is the
// FIRST maximum in genotype order, second the largest of the other nine, margin_q = best - second.  The call is the best genotype iff depth >= min_depth and
// margin_q >= min_margin_q (host::allele_min_margin_q: at least one unit, so a tie is no call), otherwise kGenotypeNoCall.  GQ = min(margin_q * 301 / 25600,
// 99) (301 / 100 ~ 10 log10 2), 0 for a no-call; PL_k = min((best - g_k) * 301 / 25600, 255).  Per contig: sites_covered, sites_deep, sites_called, called[10],
// max_depth, margin_sum_q.
#pragma once
#include "allele_core.hpp"

namespace mapad {

enum : uint32_t { GT_AA = 0, GT_CC, GT_GG, GT_TT, GT_AC, GT_AG, GT_AT, GT_CG, GT_CT, GT_GT, GT_COUNT };
constexpr uint32_t kGenotypeNoCall = 255;
constexpr uint32_t kGenotypeHets = 6;
// per-contig words of a summary
enum : uint32_t { GTC_COVERED = 0, GTC_DEEP, GTC_CALLED, GTC_CALLED_GT, GTC_MAX_DEPTH = GTC_CALLED_GT + GT_COUNT, GTC_MARGIN_SUM, GTC_WORDS };

// (GenotypeRow — one (position, quality level, read base): AC AG AT CG CT GT in read orientation, two zero words — is in common.hpp, beside Float4)

// the two alleles (0..3) of genotype g (0..9), first <= second
MAPAD_HD uint32_t genotype_allele(uint32_t g, uint32_t which) {
    if (g < 4) return g;
    const uint32_t k = g - 4;  // AC AG AT CG CT GT
    const uint32_t first = k < 3 ? 0u : k < 5 ? 1u : 2u, second = k < 3 ? k + 1 : k < 5 ? k - 1 : 3u;
    return which ? second : first;
}
// the read-orientation pair a backward record's forward-strand pair k is: both alleles complemented (AT and CG are their own complements)
MAPAD_HD uint32_t genotype_strand_pair(uint32_t k) { return k == 2 || k == 3 ? k : 5u - k; }
// the index (4..9) of the heterozygous genotype of alleles x < y
MAPAD_HD uint32_t genotype_of_pair(uint32_t x, uint32_t y) { return x == 0 ? 3u + y : x == 1 ? 5u + y : 9u; }
// the row of (position p, raw quality, read base `to` in read orientation) in a length's table (`base`: its first row)
MAPAD_HD const GenotypeRow* genotype_row_at(const GenotypeRow* table, int32_t base, uint32_t nq, uint32_t p, uint32_t qual, uint32_t to) {
    return table + (size_t)base + ((size_t)p * nq + (nq == 1 ? 0u : qual)) * 4 + to;
}
// the six values a column adds to its het cell, by forward-strand pair
MAPAD_HD void genotype_column_values(const GenotypeRow& row, bool backward, int32_t v[6]) {
#pragma unroll
    for (uint32_t k = 0; k < kGenotypeHets; ++k) v[k] = row.v[backward ? genotype_strand_pair(k) : k];  // (constant indices once unrolled: selects, no indexed load)
}

// the call of one position: 0..9 or kGenotypeNoCall; g[10]: the ten values the rule compares; best: g of the first maximum; margin_q: best - second (also
// for a no-call)
MAPAD_HD uint32_t genotype_call(const int32_t ll[4], const int32_t het[6], uint32_t depth, uint32_t min_depth, int32_t min_margin_q, int32_t het_penalty_q, int64_t g[GT_COUNT],
                                int64_t& best, int64_t& margin_q) {
#pragma unroll
    for (uint32_t a = 0; a < 4; ++a) g[a] = (int64_t)ll[a];
#pragma unroll
    for (uint32_t k = 0; k < kGenotypeHets; ++k) g[4 + k] = (int64_t)het[k] - (int64_t)het_penalty_q;
    best = g[0];
    uint32_t at = 0;
#pragma unroll
    for (uint32_t k = 1; k < GT_COUNT; ++k) if (g[k] > best) { best = g[k]; at = k; }
    int64_t second = INT64_MIN;  // the largest of the other nine
#pragma unroll
    for (uint32_t k = 0; k < GT_COUNT; ++k) if (k != at && g[k] > second) second = g[k];
    margin_q = best - second;
    return depth >= min_depth && margin_q >= (int64_t)min_margin_q ? at : kGenotypeNoCall;
}
MAPAD_HD uint32_t genotype_quality(uint32_t call, int64_t margin_q) {
    if (call == kGenotypeNoCall) return 0;
    const int64_t q = margin_q * 301 / 25600;  // (margin_q < 2^34: no overflow)
    return q > 99 ? 99u : (uint32_t)q;
}
MAPAD_HD uint32_t genotype_pl(int64_t best, int64_t g) {
    const int64_t q = (best - g) * 301 / 25600;
    return q > 255 ? 255u : (uint32_t)q;
}

// One position into the per-contig words w[GTC_WORDS] of a summary (the host path; the device keeps them in registers).
template <typename Word>
MAPAD_HD uint32_t genotype_site(const int32_t* ll, const int32_t* het, uint32_t depth, uint32_t min_depth, int32_t min_margin_q, int32_t het_penalty_q, Word* w, int64_t& margin_q) {
    int64_t g[GT_COUNT], best;
    const uint32_t call = genotype_call(ll, het, depth, min_depth, min_margin_q, het_penalty_q, g, best, margin_q);
    w[GTC_COVERED] += depth >= 1; w[GTC_DEEP] += depth >= min_depth; w[GTC_CALLED] += call != kGenotypeNoCall;
    if (call != kGenotypeNoCall) { w[GTC_CALLED_GT + call] += 1; w[GTC_MARGIN_SUM] += (Word)margin_q; }
    if ((Word)depth > w[GTC_MAX_DEPTH]) w[GTC_MAX_DEPTH] = (Word)depth;
    return call;
}

// One read on one thread (the host path): the shape and the early returns of allele_read; writes only het.  `table` / `base`: the genotype rows and the
// length's first row, base < 0 = the length has no table.  columns (may be null): += the columns added.  false: the alignment leaves [0, S] or the table is
// absent (nothing is written then).
template <typename Counter>
MAPAD_HD bool genotype_read(const CoordRec& cr, const HitRec* hits, const uint32_t* ops, const uint8_t* read, const uint8_t* quals, uint32_t L, int mode, const PileupFilter& F,
                            const GenotypeRow* table, int32_t base, uint32_t nq, uint64_t S, int32_t* het, Counter* columns, bool skip = false) {
    if (skip) return true;
    if (!damage_read_counts(cr.mapped, cr.error, cr.x0, mode)) return true;
    const HitRec& h = hits[cr.best];
    const uint32_t* t = ops + h.ops_off;
    const uint64_t abs = cr.first.abs;
    const bool backward = cr.first.backward != 0;
    if (abs > S || effective_len_hd(t, h.n_ops) > S - abs || base < 0) return false;
    uint64_t o = 0;
    for (uint32_t i = 0; i < h.n_ops; ++i) {
        const uint32_t op = coverage_ref_op(t, h.n_ops, backward, i), kind = op >> 24;
        if (kind == OP_INS) continue;
        if (kind != OP_DEL) {
            uint32_t b;
            if (pileup_column(op, read, quals, L, backward, F, b) == PIL_COUNTED) {
                const uint32_t p = op & 0xFFFFu;
                int32_t v[6];
                genotype_column_values(*genotype_row_at(table, base, nq, p, quals[p], allele_read_base(b, backward)), backward, v);
                int32_t* cell = het + (abs + o) * kGenotypeHets;
                for (uint32_t k = 0; k < kGenotypeHets; ++k) cell[k] = (int32_t)((uint32_t)cell[k] + (uint32_t)v[k]);  // (wraps like the device's atomic add)
                if (columns) *columns += 1;
            }
        }
        o += 1;
    }
    return true;
}

}  // namespace mapad
