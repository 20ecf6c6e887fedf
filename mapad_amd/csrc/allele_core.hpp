// allele_core.hpp — damage-aware consensus: per reference position, the log-likelihood (in bits) of the reported alignments' columns under each of the four
// candidate alleles A, C, G, T, with the mapper's own sequence difference model as the likelihood.  sdm_get(i, L, from, to, q) is log2 P(read base `to` | true
// base `from`, position in the read, base quality) under the user's -f / -t / -d / -s / -D; the search scores with it and DevParams::sdm_table holds it, one
// Float4 row per (position, quality level, read base) with the value for all four `from` bases: one 16-byte load per column gives that column's likelihood
// under every allele.  A deaminated T near a read's 5' end is then weak evidence against C, an interior T strong evidence, a Q2 base next to none — where the
// pileup's majority vote (pileup_core.hpp) counts them all alike.  Haploid; no prior.  One source for allele_kernel, allele_call_kernel (mapad_amd.hip), the
// host path (mapad_allele_host_*) and a stand-alone self-test (tests/emu/allele_selftest.cpp).
//
// Definition.  S = n / 2 is the forward strand's text length (coverage_core.hpp).  The accumulator is int32 ll[S][4] — forward-strand alleles A, C, G, T, in
// units of 1/256 bit — and uint32 depth[S], the columns that contributed, plus u64 scalars (the pileup's: AL_* = PIL_*).  Two arrays, so that a call reads one
// aligned 16-byte cell and one word.  Which reads and columns count is the pileup's rule, reused: damage_read_counts(cr.mapped, cr.error, cr.x0, mode); only
// hits[cr.best] at cr.first; the operations walked with coverage_ref_op, the offset o the number of non-insertion operations before the column; a Match /
// Mismatch column classified by pileup_column under this accumulator's own PileupFilter (all three values default to 0); only PIL_COUNTED columns contribute;
// deletions advance o, insertions touch nothing.  What a counted column adds, with p = op & 0xFFFF, qi the read base's index, ql = quals[p] (level 0 where the
// table has one quality level) and row = sdm_row_at(P, table_base[L], p, ql, qi), the four `from` values in READ orientation:
//     ll[abs + o][a] += allele_quantize(f4_get(row, backward ? 3 - a : a))   for a = 0..3,     depth[abs + o] += 1.
// allele_quantize(v) = saturate_i16(rintf(v * 256)) — the rule of host::dscore_quantize: the product by a power of two is exact, ties go to even; no
// transcendental is evaluated, so device and host agree bit for bit, and integer sums make the order of addition irrelevant.  A cell can wrap only beyond
// 65 536 columns of depth (65 536 * 32 768 = 2^31); that is not checked, like the pileup's counts.  Every index is checked against S before it is written: an
// alignment that leaves the text (never from record_coords) is reported, not written; so is a read whose length has no table (never for a searched read).
//
// Call rule, integers only.  best and second are the largest and the second-largest of the four cells counted with multiplicity (two equal maxima: margin 0),
// margin_q = (int64)best - second.  The call is the best allele iff depth >= min_depth and margin_q >= min_margin_q, otherwise N; min_depth >= 1, min_margin_q
// >= 1 (host_models.hpp: allele_min_margin_q), so a position nothing contributed to is N.  The quality of a call is min(margin_q >> 8, 255) whole bits, 0 for
// N.  Per contig, for a given (min_depth, min_margin_q): sites_covered (depth >= 1), sites_deep (depth >= min_depth), sites_called, called[4], max_depth and
// margin_sum_q, the sum of margin_q over the called sites.
#pragma once
#include "pileup_core.hpp"

namespace mapad {

enum : uint32_t { AL_READS = PIL_READS, AL_READS_SEEN = PIL_READS_SEEN, AL_COUNTED = PIL_COUNTED, AL_NOT_ACGT = PIL_NOT_ACGT, AL_MASKED = PIL_MASKED,
                  AL_LOW_QUAL = PIL_LOW_QUAL, AL_DELETED = PIL_DELETED, AL_INS = PIL_INS, AL_SCALARS = PIL_SCALARS };  // pileup_column's return value indexes them
// per-contig words of a summary
enum : uint32_t { ALC_COVERED = 0, ALC_DEEP, ALC_CALLED, ALC_CALLED_BASE, ALC_MAX_DEPTH = ALC_CALLED_BASE + 4, ALC_MARGIN_SUM, ALC_WORDS };

// a model value in bits -> units of 1/256 bit, saturating at the int16 range (a NaN — never from the models — lands on the lower end)
MAPAD_HD int32_t allele_quantize(float v) {
    const float x = v * 256.0f;
    if (!(x > -32768.0f)) return -32768;
    if (x >= 32767.0f) return 32767;
#if defined(__HIP_DEVICE_COMPILE__)
    return __float2int_rn(x);
#else
    return (int32_t)rintf(x);
#endif
}
// the four values a column adds to its cell, by forward-strand allele: the row holds them by `from` base in read orientation
MAPAD_HD void allele_column_values(const Float4& row, bool backward, int32_t v[4]) {
    const int32_t a = allele_quantize(row.a), c = allele_quantize(row.c), g = allele_quantize(row.g), t = allele_quantize(row.t);
    v[0] = backward ? t : a; v[1] = backward ? g : c; v[2] = backward ? c : g; v[3] = backward ? a : t;
}
// the forward-strand base pileup_column reports -> the read base's index in read orientation (the table's `to` class)
MAPAD_HD uint32_t allele_read_base(uint32_t b, bool backward) { return backward ? 3u - b : b; }

// the call of one position: 0..3 = A, C, G, T, kPileupNoCall = N; margin_q: best - second (also for N)
MAPAD_HD uint32_t allele_call(int32_t a, int32_t c, int32_t g, int32_t t, uint32_t depth, uint32_t min_depth, int32_t min_margin_q, int64_t& margin_q) {
    int32_t best = a;
    uint32_t at = 0;
    if (c > best) { best = c; at = 1; }
    if (g > best) { best = g; at = 2; }
    if (t > best) { best = t; at = 3; }
    int32_t second = INT32_MIN;  // the largest of the other three cells
    if (at != 0 && a > second) second = a;
    if (at != 1 && c > second) second = c;
    if (at != 2 && g > second) second = g;
    if (at != 3 && t > second) second = t;
    margin_q = (int64_t)best - (int64_t)second;
    return depth >= min_depth && margin_q >= (int64_t)min_margin_q ? at : kPileupNoCall;
}
MAPAD_HD uint32_t allele_quality(uint32_t call, int64_t margin_q) {
    if (call == kPileupNoCall) return 0;
    const int64_t bits = margin_q >> 8;
    return bits > 255 ? 255u : (uint32_t)bits;
}

// One position into the per-contig words w[ALC_WORDS] of a summary (the host path; the device keeps them in registers).
template <typename Word>
MAPAD_HD uint32_t allele_site(const int32_t* cell, uint32_t depth, uint32_t min_depth, int32_t min_margin_q, Word* w, int64_t& margin_q) {
    const uint32_t call = allele_call(cell[0], cell[1], cell[2], cell[3], depth, min_depth, min_margin_q, margin_q);
    w[ALC_COVERED] += depth >= 1; w[ALC_DEEP] += depth >= min_depth; w[ALC_CALLED] += call != kPileupNoCall;
    if (call != kPileupNoCall) { w[ALC_CALLED_BASE + call] += 1; w[ALC_MARGIN_SUM] += (Word)margin_q; }
    if ((Word)depth > w[ALC_MAX_DEPTH]) w[ALC_MAX_DEPTH] = (Word)depth;
    return call;
}

// One read on one thread (the host path).  `table`: DevParams::table_base[L], < 0 = the length has no table.  false: the alignment leaves [0, S] or the table
// is absent (nothing is written then).
template <typename Counter>
MAPAD_HD bool allele_read(const CoordRec& cr, const HitRec* hits, const uint32_t* ops, const uint8_t* read, const uint8_t* quals, uint32_t L, int mode, const PileupFilter& F,
                          const DevParams& P, int32_t table, uint64_t S, int32_t* ll, uint32_t* depth, Counter* scalars, bool skip = false) {
    scalars[AL_READS_SEEN] += 1;
    if (skip) return true;  // left out by mark-duplicates / damage-score mode 2: seen, not counted
    if (!damage_read_counts(cr.mapped, cr.error, cr.x0, mode)) return true;
    const HitRec& h = hits[cr.best];
    const uint32_t* t = ops + h.ops_off;
    const uint64_t abs = cr.first.abs;
    const bool backward = cr.first.backward != 0;
    if (abs > S || effective_len_hd(t, h.n_ops) > S - abs || table < 0) return false;
    scalars[AL_READS] += 1;
    uint64_t o = 0;
    for (uint32_t i = 0; i < h.n_ops; ++i) {
        const uint32_t op = coverage_ref_op(t, h.n_ops, backward, i), kind = op >> 24;
        if (kind == OP_INS) { scalars[AL_INS] += 1; continue; }
        if (kind == OP_DEL) scalars[AL_DELETED] += 1;
        else {
            uint32_t b;
            const uint32_t what = pileup_column(op, read, quals, L, backward, F, b);
            scalars[what] += 1;
            if (what == PIL_COUNTED) {
                const uint32_t p = op & 0xFFFFu;
                int32_t v[4];
                allele_column_values(sdm_row_at(P, table, (int)p, (int)quals[p], (int)allele_read_base(b, backward)), backward, v);
                int32_t* cell = ll + (abs + o) * 4;
                for (int a = 0; a < 4; ++a) cell[a] = (int32_t)((uint32_t)cell[a] + (uint32_t)v[a]);  // (wraps like the device's atomic add)
                depth[abs + o] += 1;
            }
        }
        o += 1;
    }
    return true;
}

}  // namespace mapad
