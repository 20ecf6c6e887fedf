// clean_core.hpp — per-read logic of the read clean-up ("Clean"), in integers only: a poly-G tail cut off, ends of N and of low-quality bases
// trimmed, a length test and a DUST-like complexity score, in this order and each only where its op bit is set.
//
// Two layers.  The lane functions (poly_*, run_length, dust_*) are what one lane of a wavefront computes from its own value and the ballots of the wavefront:
// clean_decide_kernel (k_clean.hpp) calls them with real ballots, tests/emu/clean_selftest.cpp with emulated ones.  decide() is the whole rule for one read on one
// thread, written straight from the specification: the host path (mapad_clean_reads_host) runs it, and the self-test holds the lanes to it.
// Written like merge_core.hpp: plain C++ that g++ compiles for the host as well.
#pragma once
#include "common.hpp"

namespace mapad {
namespace clean {

constexpr int kMaxLen = 1024;            // MAPAD_CLEAN_MAX_LEN
constexpr int kLenBins = kMaxLen + 1;    // output lengths 0 .. 1024
constexpr int kDustBins = 101;           // dust in steps of 10 permille: 0-9, 10-19, .., 990-999, 1000
enum : uint32_t { OP_POLY = 1, OP_TRIM_N = 2, OP_TRIM_QUAL = 4, OP_DUST = 8, OP_ALL = 15 };
enum : uint32_t { CLS_KEPT = 0, CLS_TRIMMED = 1, CLS_TOO_SHORT = 2, CLS_LOW_COMPLEXITY = 3, CLS_EMPTY = 4, CLS_TOO_LONG = 5, N_CLASSES = 6 };

struct Rule {  // mapad_clean_params_t as the kernels see it
    uint32_t ops, poly_base, poly_min_len, poly_one_in, poly_max_mismatch, min_quality, min_length, max_dust;
};

MAPAD_HD bool valid_base(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
MAPAD_HD bool yields_read(uint32_t cls) { return cls == CLS_KEPT || cls == CLS_TRIMMED || cls == CLS_TOO_LONG; }
MAPAD_HD int popc64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}
MAPAD_HD int ctz64(uint64_t v) {  // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((long long)v) - 1;
#else
    return __builtin_ctzll(v);
#endif
}
MAPAD_HD int clz64(uint64_t v) {  // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)v);
#else
    return __builtin_clzll(v);
#endif
}
MAPAD_HD uint64_t lanes_upto(uint32_t lane) { return lane >= 63u ? ~0ull : (1ull << (lane + 1u)) - 1ull; }  // bits 0 .. lane
MAPAD_HD uint64_t lanes_below(uint32_t lane) { return (1ull << lane) - 1ull; }                               // bits 0 .. lane - 1 (lane < 64)

// ---- poly tail: trip t, lane l looks at the n-th base from the 3' end, n = 64 t + l + 1 --------------------------------------------------------------------
// x(n) from the trip's ballot of "inside the read and not poly_base" and the mismatches of the trips before
MAPAD_HD uint32_t poly_x(uint64_t not_base, uint32_t carry, uint32_t lane) { return carry + (uint32_t)popc64(not_base & lanes_upto(lane)); }
MAPAD_HD bool poly_stop(const Rule& R, uint32_t n, uint32_t x) { return x > R.poly_max_mismatch || (n >= R.poly_min_len && (uint64_t)x * R.poly_one_in > n); }
MAPAD_HD bool poly_candidate(const Rule& R, uint32_t n, uint8_t base) { return n >= R.poly_min_len && base == (uint8_t)R.poly_base; }
// the trip's tail: the highest candidate lane below the first stop lane, as a length; 0 for none.  A lane past the read's 5' end is a stop lane.
MAPAD_HD uint32_t poly_trip_tail(uint64_t stop, uint64_t cand, uint32_t trip) {
    const uint64_t c = stop ? cand & lanes_below((uint32_t)ctz64(stop)) : cand;
    return c ? 64u * trip + (uint32_t)(63 - clz64(c)) + 1u : 0u;
}

// ---- end trimming: the run of removable lanes from lane 0 of a trip's ballot (64: the whole trip, the scan goes on) ---------------------------------------
MAPAD_HD bool removable(const Rule& R, uint8_t base, uint8_t qual) {
    return ((R.ops & OP_TRIM_N) && !valid_base(base)) || ((R.ops & OP_TRIM_QUAL) && qual != 255 && qual <= R.min_quality);
}
MAPAD_HD uint32_t run_length(uint64_t removable_lanes) { return ~removable_lanes ? (uint32_t)ctz64(~removable_lanes) : 64u; }

// ---- complexity: window k of the remainder is one trip, lane l holds the triplet that starts at base l of the window ----------------------------------------
MAPAD_HD bool dust_last_window(uint32_t k, uint32_t M) { return 32u * k + 64u >= M; }
MAPAD_HD bool dust_counted(uint32_t lane, uint32_t c0, uint32_t c1, uint32_t c2) { return lane < 62u && (c0 | c1 | c2) < 4u; }  // codes 0..3 = ACGT, 4 = anything else or no base
MAPAD_HD uint32_t dust_code(uint32_t c0, uint32_t c1, uint32_t c2) { return (c0 << 4) | (c1 << 2) | c2; }
// the counted lanes below `lane` that hold its code: B[b] = ballot of bit b of the counted lanes' codes
MAPAD_HD uint32_t dust_lane_pairs(const uint64_t B[6], uint64_t counted, uint32_t code, uint32_t lane) {
    uint64_t same = counted;
#pragma unroll
    for (int b = 0; b < 6; ++b) same &= ((code >> b) & 1u) ? B[b] : ~B[b];
    return (uint32_t)popc64(same & lanes_below(lane));
}
MAPAD_HD uint32_t dust_score(uint32_t S, uint32_t T) { return T < 2u ? 0u : 2000u * S / (T * (T - 1u)); }  // S <= 1891, T <= 62

MAPAD_HD uint32_t final_class(const Rule& R, uint32_t L, uint32_t M, uint32_t dust) {
    if (M < R.min_length) return CLS_TOO_SHORT;
    if ((R.ops & OP_DUST) && dust > R.max_dust) return CLS_LOW_COMPLEXITY;
    return M < L ? CLS_TRIMMED : CLS_KEPT;
}

// ---- the whole rule for one read on one thread ---------------------------------------------------------------------------------------------------------------
struct Decision { uint32_t cls, trim5, trim3, poly_len, dust, out_len, src; };  // the read written is r[src, src + out_len)
inline uint32_t poly_tail(const Rule& R, const uint8_t* r, uint32_t L) {
    uint32_t x = 0, tail = 0;
    for (uint32_t n = 1; n <= L; ++n) {
        x += r[L - n] != (uint8_t)R.poly_base;
        if (poly_stop(R, n, x)) break;
        if (poly_candidate(R, n, r[L - n])) tail = n;
    }
    return tail;
}
inline uint32_t window_score(const uint8_t* w, uint32_t len) {  // len <= 64
    uint32_t count[64] = {0}, T = 0, S = 0;
    for (uint32_t i = 0; i + 2 < len; ++i) {
        const uint32_t c0 = (uint32_t)base_index(w[i]), c1 = (uint32_t)base_index(w[i + 1]), c2 = (uint32_t)base_index(w[i + 2]);
        if ((c0 | c1 | c2) >= 4u) continue;
        S += count[dust_code(c0, c1, c2)]++;  // the pairs this triplet forms with the equal ones before it
        ++T;
    }
    return dust_score(S, T);
}
inline Decision decide(const Rule& R, const uint8_t* r, const uint8_t* q, uint64_t len) {
    Decision D{};
    if (len == 0) { D.cls = CLS_EMPTY; return D; }
    if (len > (uint64_t)kMaxLen) { D.cls = CLS_TOO_LONG; D.out_len = (uint32_t)(len < 0xFFFFFFFFull ? len : 0xFFFFFFFFull); return D; }
    const uint32_t L = (uint32_t)len;
    if (R.ops & OP_POLY) D.poly_len = poly_tail(R, r, L);
    uint32_t lo = 0, hi = L - D.poly_len;
    while (hi > lo && removable(R, r[hi - 1], q[hi - 1])) --hi;
    while (lo < hi && removable(R, r[lo], q[lo])) ++lo;
    D.trim5 = lo; D.trim3 = L - hi;
    const uint32_t M = hi - lo;
    if (M >= R.min_length && (R.ops & OP_DUST))
        for (uint32_t k = 0;; ++k) {
            const uint32_t b = 32u * k, e = b + 64u < M ? b + 64u : M;
            const uint32_t s = b < e ? window_score(r + lo + b, e - b) : 0u;
            D.dust = s > D.dust ? s : D.dust;
            if (dust_last_window(k, M)) break;
        }
    D.cls = final_class(R, L, M, D.dust);
    if (yields_read(D.cls)) { D.out_len = M; D.src = lo; }
    return D;
}

}  // namespace clean
}  // namespace mapad
