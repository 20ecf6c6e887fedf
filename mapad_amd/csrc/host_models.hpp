// host_models.hpp — host side of the two scoring plugins: the values the GPU tables are filled from.
//
// Mirrors trait SequenceDifferenceModel and its three impls (src/map/sequence_difference_models.rs:14-424) and trait
// MismatchBound with Discrete / Continuous / TestBound (src/map/mismatch_bounds.rs:10-281), evaluated with the same f32
// operations as the Rust code lowers to: fused fmaf for mul_add, compiler-rt style square-and-multiply for powi, glibc
// log2f / powf / expf.  Compile with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mapad_amd.h"
#include "common.hpp"

namespace mapad {
namespace host {

// f32::powi -> __powisf2
inline float powi(float a, int b) {
    const bool recip = b < 0;
    float r = 1.0f;
    for (;;) {
        if (b & 1) r *= a;
        b /= 2;
        if (b == 0) break;
        a *= a;
    }
    return recip ? 1.0f / r : r;
}
inline float qual2prob(uint8_t q) { return std::pow(10.0f, -(float)q / 10.0f) / 3.0f; }  // :275-277

inline float simple_adna_get(const mapad_params_t& p, uint64_t i, uint64_t len, uint8_t from, uint8_t to, uint8_t q) {  // :117-207
    const int fp = (int)i + 1, tp = (int)(len - 1 - i) + 1;
    const float seq_err = qual2prob(p.ignore_base_quality ? 255 : q);
    const float e = std::fmaf(seq_err, -p.divergence, seq_err + p.divergence);
    const float no_err = std::fmaf(3.0f, -e, 1.0f);
    float v = e;
    const bool ct = from == 'C' && (to == 'C' || to == 'T');
    const bool ga = from == 'G' && (to == 'G' || to == 'A');
    if ((from == 'A' && to == 'A') || (from == 'T' && to == 'T')) v = no_err;
    else if (ct || ga) {
        float p_fwd, p_rev;
        if (p.library_prep == MAPAD_LIBRARY_SINGLE_STRANDED) {
            const float f = powi(p.five_prime_overhang, fp), t = powi(p.three_prime_overhang, tp);
            p_fwd = std::fmaf(f, -t, f + t);
            p_rev = 0.0f;
        } else {
            p_fwd = powi(p.five_prime_overhang, fp);
            p_rev = powi(p.five_prime_overhang, tp);
        }
        const float pr = ct ? p_fwd : p_rev;
        const float deam = std::fmaf(p.ss_deamination_rate, pr, p.ds_deamination_rate * (1.0f - pr));
        if (to == from) v = std::fmaf(4.0f * e, deam, no_err - deam);
        else v = std::fmaf(4.0f * e, -deam, e + deam);
    }
    const float eps = 1.1920929e-07f;  // f32::EPSILON
    return std::log2(v > eps ? v : eps);
}

inline float vindija_get(uint64_t i, uint64_t len, uint8_t from, uint8_t to) {  // :357-385
    static const float ppm[7] = {0.4f, 0.25f, 0.1f, 0.06f, 0.05f, 0.04f, 0.03f};
    const float sub = 0.0005f;
    float pr;
    if (from == 'C') {
        const uint64_t k = i < len - (i + 1) ? i : len - (i + 1);
        const float ct = k < 7 ? ppm[k] : 0.02f;
        pr = to == 'T' ? ct : to == 'C' ? 1.0f - ct : sub;
    } else pr = from == to ? 1.0f - sub : sub;
    return std::log2(pr);
}

inline float sdm_get(const mapad_params_t& p, uint64_t i, uint64_t len, uint8_t from, uint8_t to, uint8_t q) {
    switch (p.model_kind) {
        case MAPAD_MODEL_SIMPLE_ADNA: return simple_adna_get(p, i, len, from, to, q);
        case MAPAD_MODEL_VINDIJA_PWM: return vindija_get(i, len, from, to);
        default: return (from == 'C' && to == 'T') ? p.deam_score : (from == to) ? p.match_score : p.mm_score;  // :415-424
    }
}
// sdm_get with the damage term removed: the null model of the damage score (dscore_core.hpp).  SimpleAncientDnaModel with both deamination rates 0; the Vindija
// matrix with its C row scored like any other base; the test model with C->T scored as a mismatch.
inline float sdm_get_null(const mapad_params_t& p, uint64_t i, uint64_t len, uint8_t from, uint8_t to, uint8_t q) {
    switch (p.model_kind) {
        case MAPAD_MODEL_SIMPLE_ADNA: {
            mapad_params_t n = p;
            n.ss_deamination_rate = 0.0f; n.ds_deamination_rate = 0.0f;
            return simple_adna_get(n, i, len, from, to, q);
        }
        case MAPAD_MODEL_VINDIJA_PWM: { const float sub = 0.0005f; return std::log2(from == to ? 1.0f - sub : sub); }
        default: return (from == to) ? p.match_score : p.mm_score;
    }
}
inline float sdm_repr_mm(const mapad_params_t& p) {  // :16-31
    return sdm_get(p, 40, 80, 'T', 'A', 255) - sdm_get(p, 40, 80, 'T', 'T', 255);
}
inline float sdm_min_penalty(const mapad_params_t& p, uint64_t i, uint64_t len, uint8_t to, uint8_t q, bool only_mm) {  // :34-57
    static const uint8_t ACGT[4] = {'A', 'C', 'G', 'T'};
    if (!only_mm && base_index(to) > 3) return 0.0f;
    float m = kF32Min;
    for (uint8_t b : ACGT) {
        if (only_mm && b == to) continue;
        const float v = sdm_get(p, i, len, b, to, q);
        m = v > m ? v : m;
    }
    return m;
}
inline int sdm_alignment_start(const mapad_params_t& p, uint64_t len) {  // :59-61, :209-211
    return p.model_kind == MAPAD_MODEL_SIMPLE_ADNA ? (int)(int16_t)len : (int)((int16_t)len / 2);
}

// Discrete::calculate_max_num_mismatches (mismatch_bounds.rs:217-241)
inline float discrete_allowed(uint64_t len, float thr, float err) {
    if (len < 17) return 0.0f;  // :245-247
    const float lambda = (float)len * err;
    const float eml = std::exp(-lambda);
    if (!(1.0f - eml > thr)) return 0.0f;
    uint64_t last = 1, fact = 1;
    float pw = 1.0f, sum = eml;
    for (uint64_t k = 1; k <= len; ++k) {
        pw *= lambda;
        fact *= k;
        sum += pw * eml / (float)fact;
        if (1.0f - sum > thr) last = k + 1; else break;
    }
    return (float)last;
}
inline float bound_repr_mm(const mapad_params_t& p) { return p.bound_kind == MAPAD_BOUND_TEST ? p.repr_mm_bound : sdm_repr_mm(p); }
// the per-length quantity the kernels compare against (common.hpp: DevParams::reject_thr)
inline float bound_threshold(const mapad_params_t& p, uint64_t len, float repr_mm) {
    switch (p.bound_kind) {
        case MAPAD_BOUND_DISCRETE: return discrete_allowed(len, p.poisson_threshold, p.base_error_rate) * repr_mm;  // :131-134
        case MAPAD_BOUND_CONTINUOUS: return std::pow((float)len, p.exponent);                                       // :107-119
        default: return p.threshold;
    }
}
inline bool mb_reject(const mapad_params_t& p, float v, uint64_t len) {
    const float t = bound_threshold(p, len, bound_repr_mm(p));
    return p.bound_kind == MAPAD_BOUND_CONTINUOUS ? (v / t) < p.cutoff : v < t;
}
inline bool mb_reject_iterative(const mapad_params_t& p, float v, float ref) {
    return p.bound_kind == MAPAD_BOUND_TEST ? false : v < ref + bound_repr_mm(p);
}
inline float mb_remaining_frac(const mapad_params_t& p, float v, uint64_t len) {  // :93-98, :140-144, :277-279
    const float repr = bound_repr_mm(p);
    switch (p.bound_kind) {
        case MAPAD_BOUND_DISCRETE: return std::fmaf(discrete_allowed(len, p.poisson_threshold, p.base_error_rate), repr, -v) / repr;
        case MAPAD_BOUND_CONTINUOUS: { const float s = std::pow((float)len, p.exponent); return (p.cutoff - v / s) / (repr / s); }
        default: return (p.threshold - v) / p.repr_mm_bound;
    }
}

// ---- tables the kernels read (common.hpp: DevParams) --------------------------------------------------------------------
struct HostTables {
    int nq = 1;                       // quality levels per position
    std::vector<int32_t> table_base;  // [kMaxReadLen + 1], -1 = absent
    std::vector<float> sdm;           // float4 entries
    std::vector<float> reject_thr;    // [kMaxReadLen + 1]
    float repr_mm = 0;
};
inline int quality_levels(const mapad_params_t& p) {
    return (p.model_kind == MAPAD_MODEL_SIMPLE_ADNA && !p.ignore_base_quality) ? 256 : 1;
}
// appends the table of one read length (all positions x quality levels x 5 read-base classes x 4 reference bases)
inline void add_length(const mapad_params_t& p, HostTables& t, int len) {
    if (t.table_base[len] >= 0) return;
    static const uint8_t TO[5] = {'A', 'C', 'G', 'T', 'N'}, FROM[4] = {'A', 'C', 'G', 'T'};
    t.table_base[len] = (int32_t)(t.sdm.size() / 4);
    const size_t base = t.sdm.size();
    t.sdm.resize(base + (size_t)len * t.nq * 5 * 4);
    // SimpleAncientDnaModel: the value depends on q only through qual2prob(q); positions only matter for C/G rows
    for (int i = 0; i < len; ++i)
        for (int q = 0; q < t.nq; ++q)
            for (int c = 0; c < 5; ++c)
                for (int f = 0; f < 4; ++f)
                    t.sdm[base + ((((size_t)i * t.nq + q) * 5 + c) * 4) + f] = sdm_get(p, (uint64_t)i, (uint64_t)len, FROM[f], TO[c], (uint8_t)q);
}
// ---- damage score (dscore_core.hpp): the rounding rules and the table, on the host with libm like every other table ----
// a difference of two model values in bits -> units of 1/256 bit: the product is exact (a power of two), ties round to even, the result saturates
inline int16_t dscore_quantize(float diff) {
    const float v = std::rint(diff * 256.0f);
    if (!(v > -32768.0f)) return (int16_t)-32768;  // (a NaN — never from the models — lands here)
    if (v >= 32767.0f) return (int16_t)32767;
    return (int16_t)v;
}
// the threshold in the same units; false: not a number
inline bool dscore_threshold_q(float threshold, int32_t& thr_q) {
    if (threshold != threshold) return false;
    const float v = std::ceil(threshold * 256.0f);
    thr_q = v >= 2147483648.0f ? INT32_MAX : v <= -2147483648.0f ? INT32_MIN : (int32_t)v;
    return true;
}
// allele likelihoods (allele_core.hpp): the smallest margin a call needs, in the same units and by the same rounding, at least one unit; false: not a number
inline bool allele_min_margin_q(float min_margin_bits, int32_t& min_margin_q) {
    if (!dscore_threshold_q(min_margin_bits, min_margin_q)) return false;
    if (min_margin_q < 1) min_margin_q = 1;
    return true;
}
// appends one read length's table int16 [len][nq][4] — C->C, C->T, G->G, G->A; every other pair is equal under both models — to `out`
inline void dscore_table(const mapad_params_t& p, int len, int nq, std::vector<int16_t>& out) {
    static const uint8_t FROM[4] = {'C', 'C', 'G', 'G'}, TO[4] = {'C', 'T', 'G', 'A'};
    const size_t base = out.size();
    out.resize(base + (size_t)len * nq * 4);
    for (int i = 0; i < len; ++i)
        for (int q = 0; q < nq; ++q)
            for (int c = 0; c < 4; ++c) {
                const float with = sdm_get(p, (uint64_t)i, (uint64_t)len, FROM[c], TO[c], (uint8_t)q), without = sdm_get_null(p, (uint64_t)i, (uint64_t)len, FROM[c], TO[c], (uint8_t)q);
                out[base + ((size_t)i * nq + q) * 4 + c] = dscore_quantize(with - without);
            }
}
// ---- quality rescaling (rescale_core.hpp) ----
// The model's LINEAR probability of a column, with (`null` false: what sdm_get takes the log of) or without (what sdm_get_null does) the damage term: before the
// log and before the epsilon clamp, in double from the f32 parameters.  SimpleAncientDnaModel: the v of simple_adna_get, deam = 0 for null, quality 255 inside
// the model under ignore_base_quality as the model itself does; the Vindija matrix entry, or sub for null; the test model: exp2(score).
inline double sdm_prob(const mapad_params_t& p, uint64_t i, uint64_t len, uint8_t from, uint8_t to, uint8_t q, bool null) {
    switch (p.model_kind) {
        case MAPAD_MODEL_SIMPLE_ADNA: {
            const int fp = (int)i + 1, tp = (int)(len - 1 - i) + 1;
            const double div = (double)p.divergence;
            const double seq_err = std::pow(10.0, -(double)(p.ignore_base_quality ? 255 : q) / 10.0) / 3.0;
            const double e = seq_err + div - seq_err * div;
            const double no_err = 1.0 - 3.0 * e;
            const bool ct = from == 'C' && (to == 'C' || to == 'T');
            const bool ga = from == 'G' && (to == 'G' || to == 'A');
            if ((from == 'A' && to == 'A') || (from == 'T' && to == 'T')) return no_err;
            if (!ct && !ga) return e;
            double deam = 0.0;
            if (!null) {
                const double f5 = (double)p.five_prime_overhang, f3 = (double)p.three_prime_overhang;
                double p_fwd, p_rev;
                if (p.library_prep == MAPAD_LIBRARY_SINGLE_STRANDED) {
                    const double f = std::pow(f5, fp), t = std::pow(f3, tp);
                    p_fwd = f + t - f * t;
                    p_rev = 0.0;
                } else {
                    p_fwd = std::pow(f5, fp);
                    p_rev = std::pow(f5, tp);
                }
                const double pr = ct ? p_fwd : p_rev;
                deam = (double)p.ss_deamination_rate * pr + (double)p.ds_deamination_rate * (1.0 - pr);
            }
            return to == from ? no_err - deam + 4.0 * e * deam : e + deam - 4.0 * e * deam;
        }
        case MAPAD_MODEL_VINDIJA_PWM: {
            static const float ppm[7] = {0.4f, 0.25f, 0.1f, 0.06f, 0.05f, 0.04f, 0.03f};
            const double sub = (double)0.0005f;
            if (null || from != 'C') return from == to ? 1.0 - sub : sub;
            const uint64_t k = i < len - (i + 1) ? i : len - (i + 1);
            const double ct = (double)(k < 7 ? ppm[k] : 0.02f);
            return to == 'T' ? ct : to == 'C' ? 1.0 - ct : sub;
        }
        default: return std::exp2((double)(null ? sdm_get_null(p, i, len, from, to, q) : sdm_get(p, i, len, from, to, q)));
    }
}
// one table entry: the quality byte q (0..254) of a C->T (cell 0) or G->A (cell 1) mismatch at position i, marked down by the posterior that it is damage
inline uint8_t rescale_quality(const mapad_params_t& p, int i, int len, int cell, int q) {
    const uint8_t from = cell == 0 ? 'C' : 'G', to = cell == 0 ? 'T' : 'A';
    const double p_dam = sdm_prob(p, (uint64_t)i, (uint64_t)len, from, to, (uint8_t)q, false), p_null = sdm_prob(p, (uint64_t)i, (uint64_t)len, from, to, (uint8_t)q, true);
    double pd = p_dam > 0.0 ? (p_dam - p_null) / p_dam : 0.0;
    pd = !(pd > 0.0) ? 0.0 : pd > 1.0 ? 1.0 : pd;
    if (pd == 0.0) return (uint8_t)q;  // e' = e
    const double e = std::pow(10.0, -(double)q / 10.0);
    const double e2 = 1.0 - (1.0 - e) * (1.0 - pd);
    if (e2 >= 1.0) return 0;
    if (!(e2 > 0.0)) return (uint8_t)q;  // (pd below half an ulp of 1 and e below it too: nothing left of either)
    const double nq = std::floor(-10.0 * std::log10(e2) + 0.5);
    return nq >= (double)q ? (uint8_t)q : nq <= 0.0 ? (uint8_t)0 : (uint8_t)nq;
}
// appends one read length's table uint8 [len][256][2] — C->T, G->A — to `out`; the row of the missing quality 255 holds 255
inline void rescale_table(const mapad_params_t& p, int len, std::vector<uint8_t>& out) {
    const size_t base = out.size();
    out.resize(base + (size_t)len * 512);
    for (int i = 0; i < len; ++i)
        for (int q = 0; q < 256; ++q)
            for (int c = 0; c < 2; ++c) out[base + ((size_t)i * 256 + q) * 2 + c] = q == 255 ? (uint8_t)255 : rescale_quality(p, i, len, c, q);
}
// genotype likelihoods (genotype_core.hpp): what a column of read base `to` is worth under the heterozygous pair {x, y} of true bases in read orientation,
// log2(0.5 * 2^s_x + 0.5 * 2^s_y), in double from the two f32 model values, then f32 and the rounding above (a sum of 0 or a NaN lands on the lower end)
inline int16_t genotype_pair_from_powers(double px, double py) {  // px = 2^s_x, py = 2^s_y
    const double sum = 0.5 * px + 0.5 * py;
    return dscore_quantize(sum > 0.0 ? (float)std::log2(sum) : -std::numeric_limits<float>::infinity());
}
inline int16_t genotype_pair_quantized(float s_x, float s_y) { return genotype_pair_from_powers(std::exp2((double)s_x), std::exp2((double)s_y)); }
// one row: the pairs AC AG AT CG CT GT from the four model values by true base A, C, G, T, then two zero words
inline void genotype_row(const float s[4], GenotypeRow& row) {
    static const int X[6] = {0, 0, 0, 1, 1, 2}, Y[6] = {1, 2, 3, 2, 3, 3};
    double pw[4];
    for (int f = 0; f < 4; ++f) pw[f] = std::exp2((double)s[f]);
    for (int k = 0; k < 6; ++k) row.v[k] = genotype_pair_from_powers(pw[X[k]], pw[Y[k]]);
    row.v[6] = row.v[7] = 0;
}
// appends one read length's table GenotypeRow [len][nq][4 read bases] (int16 [..][8]) — the pairs AC AG AT CG CT GT by `from` pair in read orientation, two zero words — to `out`,
// from that length's score table `sdm` as add_length lays it out ([len][nq][5 read-base classes][4 true bases]: the same f32 values sdm_get returns)
inline void genotype_table_from(const float* sdm, int len, int nq, std::vector<GenotypeRow>& out) {
    const size_t base = out.size();
    out.resize(base + (size_t)len * nq * 4);
    for (int i = 0; i < len; ++i)
        for (int q = 0; q < nq; ++q)
            for (int c = 0; c < 4; ++c) {
                const float* s = sdm + (((size_t)i * nq + q) * 5 + c) * 4;
                GenotypeRow& row = out[base + ((size_t)i * nq + q) * 4 + c];
                // most rows do not depend on the position, and a row costs ten libm calls: the row of the position before where its model values are the same
                if (i > 0 && std::memcmp(s - (size_t)nq * 5 * 4, s, 4 * sizeof(float)) == 0) row = *(&row - (size_t)nq * 4);
                else genotype_row(s, row);
            }
}
// the same from the parameters alone
inline void genotype_table(const mapad_params_t& p, int len, int nq, std::vector<GenotypeRow>& out) {
    HostTables t;
    t.nq = nq;
    t.table_base.assign(kMaxReadLen + 1, -1);
    add_length(p, t, len);
    genotype_table_from(t.sdm.data(), len, nq, out);
}
inline HostTables make_tables(const mapad_params_t& p) {
    HostTables t;
    t.nq = quality_levels(p);
    t.table_base.assign(kMaxReadLen + 1, -1);
    t.repr_mm = bound_repr_mm(p);
    t.reject_thr.resize(kMaxReadLen + 1);
    for (int l = 0; l <= kMaxReadLen; ++l) t.reject_thr[l] = bound_threshold(p, (uint64_t)l, t.repr_mm);
    return t;
}

}  // namespace host
}  // namespace mapad
