// merge_core.hpp — per-pair logic of adapter trimming and read-pair merging ("Trim and merge"), in integers only.
//
// Mate 1 (r1, q1, L1) and mate 2 (r2, q2, L2) as sequenced, adapters A1 / A2 behind the fragment in mate 1 / mate 2.  A candidate is a fragment length F; its
// columns are the overlap of r1 with revcomp(r2) laid F wide, plus what follows the fragment in either mate against that mate's adapter.  With
//     X = revcomp(A2) ++ r1            Y = revcomp(r2) ++ A1
// every column of candidate F is X[i] against Y[i + d], d = L2 - F - |A2|, for every i both strings have: one shifted Hamming compare (the adapters never face
// each other because F >= 0).  So X and Y are packed once per pair into bit planes — two code bits and a valid bit per base, 64 bases per word — and a candidate
// costs a few funnel-shifted words, XOR, AND and popcount per 64 columns instead of a loop over bases (mapad_amd.hip: merge_decide_kernel, a candidate per lane).
// Single-end trimming is the same with mate 2 and A2 empty: X = r1, Y = A1.
// Written like collapse_core.hpp and align_core.hpp: plain C++ that g++ compiles for the host as well — the kernels, the host path (mapad_merge_pairs_host) and
// tests/emu/merge_selftest.cpp run these very functions.
#pragma once
#include "common.hpp"

namespace mapad {
namespace merge {

constexpr int kMaxMate = 512;     // MAPAD_MERGE_MAX_MATE_LEN
constexpr int kMaxAdapter = 64;   // MAPAD_MERGE_MAX_ADAPTER
constexpr int kPlaneWords = (kMaxMate + kMaxAdapter + 63) / 64;  // 9 words per plane
constexpr int kHistBins = 2 * kMaxMate + 1;                       // fragment lengths 0 .. 1024
enum : uint32_t { CLS_MERGED = 0, CLS_TOO_SHORT = 1, CLS_UNMERGED = 2, CLS_EMPTY_MATE = 3, CLS_TOO_LONG = 4, N_CLASSES = 5 };  // single-end: trimmed, too_short, untouched, empty, too_long
enum : uint32_t { MODE_PAIRS = 0, MODE_SINGLE = 1 };

struct Rule {  // mapad_merge_params_t as the kernels see it
    uint32_t min_overlap;  // pairs: min_overlap; single-end: min_adapter_overlap
    uint32_t max_mismatch_permille, min_length, max_quality, mode;
    uint32_t a1_len, a2_len;
    uint8_t a1[kMaxAdapter], a2[kMaxAdapter];
};

MAPAD_HD bool valid_base(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
MAPAD_HD uint8_t comp(uint8_t c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }
// two code bits and a valid bit: A=4 C=5 G=6 T=7, everything else 0
MAPAD_HD uint32_t code3(uint8_t c) { const int b = base_index(c); return b < 4 ? 4u | (uint32_t)b : 0u; }

// the byte of X = revcomp(A2) ++ r1 at index i, of Y = revcomp(r2) ++ A1 at index j (0 = none, which packs as invalid)
MAPAD_HD uint8_t x_byte(const Rule& R, const uint8_t* r1, int L1, int i) {
    const int a2 = (int)R.a2_len;
    if (i < a2) return comp(R.a2[a2 - 1 - i]);
    return i < a2 + L1 ? r1[i - a2] : (uint8_t)0;
}
MAPAD_HD uint8_t y_byte(const Rule& R, const uint8_t* r2, int L2, int j) {
    if (j < L2) return comp(r2[L2 - 1 - j]);
    return j < L2 + (int)R.a1_len ? R.a1[j - L2] : (uint8_t)0;
}

// the planes of one string: bit (i & 63) of word (i >> 6) belongs to index i
struct Planes {
    uint64_t c0[kPlaneWords], c1[kPlaneWords], v[kPlaneWords];
};

// words [q, q + 1] of a plane as the 64 bits that start at bit 64 q + b (0 <= b < 64); words outside [0, kPlaneWords) are zero
MAPAD_HD uint64_t plane_word(const uint64_t* pl, int q) { return (q >= 0 && q < kPlaneWords) ? pl[q] : 0ull; }
MAPAD_HD uint64_t funnel(const uint64_t* pl, int q, int b) {
    const uint64_t lo = plane_word(pl, q);
    if (b == 0) return lo;
    return (lo >> b) | (plane_word(pl, q + 1) << (64 - b));
}
MAPAD_HD int popc64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}

// the highest candidate, or -1 for none
MAPAD_HD int max_candidate(const Rule& R, int L1, int L2) { return L1 + L2 - (int)R.min_overlap; }

// (m, x) of candidate F from the planes of X and Y
MAPAD_HD void candidate_counts(const Planes& X, const Planes& Y, const Rule& R, int L1, int L2, int F, int& m, int& x) {
    const int d = L2 - F - (int)R.a2_len;  // Y index = X index + d
    const int q0 = d >> 6, b = d & 63;     // floor division: d may be negative
    const int nx = ((int)R.a2_len + L1 + 63) >> 6;
    m = 0; x = 0;
    for (int w = 0; w < nx; ++w) {
        const uint64_t valid = X.v[w] & funnel(Y.v, q0 + w, b);
        if (!valid) continue;
        const uint64_t diff = (X.c0[w] ^ funnel(Y.c0, q0 + w, b)) | (X.c1[w] ^ funnel(Y.c1, q0 + w, b));
        x += popc64(valid & diff);
        m += popc64(valid & ~diff);
    }
}

MAPAD_HD bool admissible(const Rule& R, int m, int x) {
    const uint32_t n = (uint32_t)(m + x);
    return n >= R.min_overlap && (uint32_t)x * 1000u <= n * R.max_mismatch_permille;
}
// what the choice maximises: m - x first, the smaller F second; 0 = not admissible (an admissible key is never 0: its low half is at least 0xFFFF - 1024)
MAPAD_HD uint32_t order_key(const Rule& R, int F, int m, int x) {
    if (!admissible(R, m, x)) return 0u;
    return ((uint32_t)(m - x + 0x8000) << 16) | (0xFFFFu - (uint32_t)F);
}
MAPAD_HD int key_frag_len(uint32_t key) { return (int)(0xFFFFu - (key & 0xFFFFu)); }

// the class decided before any compare, or N_CLASSES for "compare"
MAPAD_HD uint32_t early_class(const Rule& R, int L1, int L2) {
    const bool single = R.mode == MODE_SINGLE;
    if (L1 == 0 || (!single && L2 == 0)) return CLS_EMPTY_MATE;
    if (L1 > kMaxMate || L2 > kMaxMate) return CLS_TOO_LONG;
    return N_CLASSES;
}
// whether a pair of this class puts a read into the output (pairs: merged; single-end: trimmed and untouched)
MAPAD_HD bool yields_read(const Rule& R, uint32_t cls) { return cls == CLS_MERGED || (R.mode == MODE_SINGLE && cls == CLS_UNMERGED); }
// class and output length from the winning key (0 = none).  Single-end: what is left of the read — r1[0, F), or all of it — is too_short below min_length
MAPAD_HD uint32_t final_class(const Rule& R, int L1, uint32_t key, int& out_len) {
    const bool single = R.mode == MODE_SINGLE;
    const int len = key ? key_frag_len(key) : (single ? L1 : 0);
    uint32_t cls;
    if (key || single) cls = (uint32_t)len < R.min_length ? (uint32_t)CLS_TOO_SHORT : key ? (uint32_t)CLS_MERGED : (uint32_t)CLS_UNMERGED;
    else cls = CLS_UNMERGED;
    out_len = yields_read(R, cls) ? len : 0;
    return cls;
}

// output column p of the merged read of fragment length F (single-end: of r1[0, F))
MAPAD_HD void column(const Rule& R, const uint8_t* r1, const uint8_t* q1, int L1, const uint8_t* r2, const uint8_t* q2, int L2, int F, int p, uint8_t& base, uint8_t& qual) {
    if (R.mode == MODE_SINGLE) { base = r1[p]; qual = q1[p]; return; }
    const int lo = F - L2 > 0 ? F - L2 : 0, hi = F < L1 ? F : L1;
    if (p < lo) { base = r1[p]; qual = q1[p]; return; }
    if (p >= hi) { base = comp(r2[F - 1 - p]); qual = q2[F - 1 - p]; return; }
    const uint8_t b1 = r1[p], b2 = comp(r2[F - 1 - p]), y1 = q1[p], y2 = q2[F - 1 - p];
    const uint32_t h1 = y1 == 255 ? 0u : y1, h2 = y2 == 255 ? 0u : y2;
    const bool v1 = valid_base(b1), v2 = valid_base(b2);
    if (!v1 && !v2) { base = 'N'; qual = 0; }
    else if (!v2) { base = b1; qual = y1; }
    else if (!v1) { base = b2; qual = y2; }
    else if (b1 == b2) { const uint32_t s = h1 + h2; base = b1; qual = (uint8_t)(s < R.max_quality ? s : R.max_quality); }
    else if (h1 == h2) { base = 'N'; qual = 0; }
    else if (h1 > h2) { base = b1; qual = (uint8_t)(h1 - h2); }
    else { base = b2; qual = (uint8_t)(h2 - h1); }
    if (y1 == 255 && y2 == 255) qual = 255;
}

// ---- the whole rule for one pair on one thread (the host path; the kernels spread the same calls over a wavefront) ----------------------------------------
MAPAD_HD void pack_bit(Planes& P, int i, uint8_t byte) {
    const uint32_t c = code3(byte);
    const uint64_t bit = 1ull << (i & 63);
    if (c & 1u) P.c0[i >> 6] |= bit;
    if (c & 2u) P.c1[i >> 6] |= bit;
    if (c & 4u) P.v[i >> 6] |= bit;
}
struct Decision { uint32_t cls; int32_t frag_len; uint32_t m, x; int out_len; };
inline Decision decide(const Rule& R, const uint8_t* r1, int L1, const uint8_t* r2, int L2) {
    Decision D{early_class(R, L1, L2), -1, 0, 0, 0};
    if (D.cls != N_CLASSES) return D;
    Planes X{}, Y{};
    for (int i = 0; i < (int)R.a2_len + L1; ++i) pack_bit(X, i, x_byte(R, r1, L1, i));
    for (int j = 0; j < L2 + (int)R.a1_len; ++j) pack_bit(Y, j, y_byte(R, r2, L2, j));
    uint32_t best = 0, bm = 0, bx = 0;
    for (int F = 0; F <= max_candidate(R, L1, L2); ++F) {
        int m, x;
        candidate_counts(X, Y, R, L1, L2, F, m, x);
        const uint32_t key = order_key(R, F, m, x);
        if (key > best) { best = key; bm = (uint32_t)m; bx = (uint32_t)x; }
    }
    D.cls = final_class(R, L1, best, D.out_len);
    if (best) { D.frag_len = key_frag_len(best); D.m = bm; D.x = bx; }
    return D;
}

}  // namespace merge
}  // namespace mapad
