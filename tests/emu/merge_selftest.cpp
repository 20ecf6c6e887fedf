// merge_selftest.cpp — merge_core.hpp driven the way merge_decide_kernel drives it, against a byte-by-byte serial restatement of the rule.
// 64 emulated lanes: the planes of X and Y are built by ballots over the lanes' codes (64 indices per trip), lane l takes the candidates F = l + 64 t, the winner
// is the maximum of the lanes' keys; merge_write_kernel's columns are merge::column.  Checked: (m, x) of every candidate, the decision and the merged bytes,
// over random pairs (mates of 1 .. 512 bases with N and IUPAC bytes, adapters of 0 .. 64, fragments planted or not) and every shift across the word boundaries.
// Stand-alone (own main), built with -fsanitize=address,undefined by tests/test_merge_host.py: every index the core forms is checked on the way.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../mapad_amd/csrc/merge_core.hpp"

using namespace mapad;
typedef std::vector<uint8_t> Bytes;

static bool valid(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
static uint8_t cmp(uint8_t c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }

// ---- the serial restatement -------------------------------------------------------------------------------------------------------------------------------
static void serial_counts(const Bytes& r1, const Bytes& r2, const Bytes& a1, const Bytes& a2, int F, int& m, int& x) {
    const int L1 = (int)r1.size(), L2 = (int)r2.size();
    m = x = 0;
    auto col = [&](uint8_t a, uint8_t b) { if (valid(a) && valid(b)) { if (a == b) ++m; else ++x; } };
    for (int p = std::max(0, F - L2); p < std::min(F, L1); ++p) col(r1[p], cmp(r2[F - 1 - p]));
    if (F < L1) for (int k = 0; k < std::min(L1 - F, (int)a1.size()); ++k) col(r1[F + k], a1[k]);
    if (F < L2) for (int k = 0; k < std::min(L2 - F, (int)a2.size()); ++k) col(r2[F + k], a2[k]);
}
struct Serial { bool chosen; int F, m, x; };
static Serial serial_choose(const Bytes& r1, const Bytes& r2, const Bytes& a1, const Bytes& a2, int min_overlap, int permille) {
    Serial best{false, -1, 0, 0};
    for (int F = 0; F <= (int)r1.size() + (int)r2.size() - min_overlap; ++F) {
        int m, x;
        serial_counts(r1, r2, a1, a2, F, m, x);
        const int n = m + x;
        if (n >= min_overlap && x * 1000 <= n * permille && (!best.chosen || m - x > best.m - best.x)) best = Serial{true, F, m, x};
    }
    return best;
}
static void serial_column(const Bytes& r1, const Bytes& q1, const Bytes& r2, const Bytes& q2, int F, int p, int max_quality, uint8_t& b, uint8_t& q) {
    const int L1 = (int)r1.size(), L2 = (int)r2.size();
    if (p < std::max(0, F - L2)) { b = r1[p]; q = q1[p]; return; }
    if (p >= std::min(F, L1)) { b = cmp(r2[F - 1 - p]); q = q2[F - 1 - p]; return; }
    const uint8_t b1 = r1[p], b2 = cmp(r2[F - 1 - p]), y1 = q1[p], y2 = q2[F - 1 - p];
    const int h1 = y1 == 255 ? 0 : y1, h2 = y2 == 255 ? 0 : y2;
    if (!valid(b1) && !valid(b2)) { b = 'N'; q = 0; }
    else if (!valid(b2)) { b = b1; q = y1; }
    else if (!valid(b1)) { b = b2; q = y2; }
    else if (b1 == b2) { b = b1; q = (uint8_t)std::min(h1 + h2, max_quality); }
    else if (h1 == h2) { b = 'N'; q = 0; }
    else if (h1 > h2) { b = b1; q = (uint8_t)(h1 - h2); }
    else { b = b2; q = (uint8_t)(h2 - h1); }
    if (y1 == 255 && y2 == 255) q = 255;
}

// ---- the kernel's way --------------------------------------------------------------------------------------------------------------------------------------
static uint64_t ballot(const bool pred[64]) { uint64_t m = 0; for (int l = 0; l < 64; ++l) if (pred[l]) m |= 1ull << l; return m; }
static void wave_pack(const merge::Rule& R, const uint8_t* r1, int L1, const uint8_t* r2, int L2, merge::Planes& X, merge::Planes& Y) {
    const int nx = (int)R.a2_len + L1, ny = L2 + (int)R.a1_len;
    for (int w = 0; w < merge::kPlaneWords; ++w) {
        bool p[6][64];
        for (int lane = 0; lane < 64; ++lane) {
            const int i = 64 * w + lane;
            const uint32_t cx = i < nx ? merge::code3(merge::x_byte(R, r1, L1, i)) : 0u, cy = i < ny ? merge::code3(merge::y_byte(R, r2, L2, i)) : 0u;
            p[0][lane] = cx & 1u; p[1][lane] = cx & 2u; p[2][lane] = cx & 4u; p[3][lane] = cy & 1u; p[4][lane] = cy & 2u; p[5][lane] = cy & 4u;
        }
        X.c0[w] = ballot(p[0]); X.c1[w] = ballot(p[1]); X.v[w] = ballot(p[2]); Y.c0[w] = ballot(p[3]); Y.c1[w] = ballot(p[4]); Y.v[w] = ballot(p[5]);
    }
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static merge::Rule make_rule(const Bytes& a1, const Bytes& a2, uint32_t min_overlap, uint32_t permille, uint32_t min_length, uint32_t max_quality, uint32_t mode) {
    merge::Rule R{};
    R.min_overlap = min_overlap; R.max_mismatch_permille = permille; R.min_length = min_length; R.max_quality = max_quality; R.mode = mode;
    R.a1_len = (uint32_t)a1.size(); R.a2_len = (uint32_t)a2.size();
    for (size_t k = 0; k < a1.size(); ++k) R.a1[k] = a1[k];
    for (size_t k = 0; k < a2.size(); ++k) R.a2[k] = a2[k];
    return R;
}

static void check_pair(const merge::Rule& R, const Bytes& r1, const Bytes& q1, const Bytes& r2, const Bytes& q2, const Bytes& a1, const Bytes& a2, const char* what) {
    const int L1 = (int)r1.size(), L2 = (int)r2.size();
    // exactly-sized copies: an index past a mate is the sanitizer's to find
    merge::Planes X{}, Y{};
    wave_pack(R, r1.data(), L1, r2.data(), L2, X, Y);
    uint32_t lane_key[64] = {0}, lane_m[64] = {0}, lane_x[64] = {0};
    const int fmax = merge::max_candidate(R, L1, L2);
    for (int lane = 0; lane < 64; ++lane)
        for (int F = lane; F <= fmax; F += 64) {
            int m, x, sm, sx;
            merge::candidate_counts(X, Y, R, L1, L2, F, m, x);
            serial_counts(r1, r2, a1, a2, F, sm, sx);
            CHECK(m == sm && x == sx, "%s: L1 %d L2 %d a1 %zu a2 %zu F %d: (m, x) = (%d, %d), serial (%d, %d)", what, L1, L2, a1.size(), a2.size(), F, m, x, sm, sx);
            const uint32_t k = merge::order_key(R, F, m, x);
            if (k > lane_key[lane]) { lane_key[lane] = k; lane_m[lane] = (uint32_t)m; lane_x[lane] = (uint32_t)x; }
        }
    uint32_t best = 0; int owner = -1;
    for (int lane = 0; lane < 64; ++lane) if (lane_key[lane] > best) { best = lane_key[lane]; owner = lane; }
    const Serial S = serial_choose(r1, r2, a1, a2, (int)R.min_overlap, (int)R.max_mismatch_permille);
    CHECK((best != 0) == S.chosen, "%s: chosen %d, serial %d", what, best != 0, S.chosen);
    if (best && S.chosen) {
        CHECK(merge::key_frag_len(best) == S.F && (int)lane_m[owner] == S.m && (int)lane_x[owner] == S.x, "%s: L1 %d L2 %d: F %d (m %u x %u), serial F %d (m %d x %d)", what,
              L1, L2, merge::key_frag_len(best), lane_m[owner], lane_x[owner], S.F, S.m, S.x);
        int out_len = 0;
        const uint32_t cls = merge::final_class(R, L1, best, out_len);
        CHECK(cls == (S.F < (int)R.min_length ? merge::CLS_TOO_SHORT : merge::CLS_MERGED), "%s: class %u at F %d", what, cls, S.F);
        if (R.mode == merge::MODE_PAIRS)
            for (int p = 0; p < out_len; ++p) {
                uint8_t b, q, sb, sq;
                merge::column(R, r1.data(), q1.data(), L1, r2.data(), q2.data(), L2, S.F, p, b, q);
                serial_column(r1, q1, r2, q2, S.F, p, (int)R.max_quality, sb, sq);
                CHECK(b == sb && q == sq, "%s: F %d column %d: %c/%u, serial %c/%u", what, S.F, p, b, q, sb, sq);
            }
    }
    // the one-thread driver of the host path agrees with the lanes
    const merge::Decision D = merge::decide(R, r1.data(), L1, r2.data(), L2);
    CHECK((D.frag_len >= 0) == (best != 0) && (!best || D.frag_len == merge::key_frag_len(best)), "%s: decide() says F %d", what, D.frag_len);
}

int main() {
    std::mt19937_64 rng(12345);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    auto bases = [&](int n, int dirty_permille) {
        Bytes s((size_t)n);
        for (auto& c : s) { c = (uint8_t)"ACGT"[rng() & 3]; if (rnd(0, 999) < dirty_permille) c = (uint8_t)"NRYacgt."[rng() & 7]; }
        return s;
    };
    auto quals = [&](int n) { Bytes q((size_t)n); for (auto& c : q) { const int k = rnd(0, 9); c = k == 0 ? 255 : k == 1 ? 0 : k == 2 ? 93 : (uint8_t)rnd(2, 41); } return q; };
    auto revcomp = [&](const Bytes& s) { Bytes o(s.rbegin(), s.rend()); for (auto& c : o) c = cmp(c); return o; };
    auto sequenced = [&](const Bytes& frag, const Bytes& adapter, int L) {
        Bytes t = frag; t.insert(t.end(), adapter.begin(), adapter.end());
        const Bytes tail = bases(L, 0); t.insert(t.end(), tail.begin(), tail.end());
        t.resize((size_t)L);
        return t;
    };
    const Bytes A1{'A','G','A','T','C','G','G','A','A','G','A','G','C','A','C','A','C','G','T','C','T','G','A','A','C','T','C','C','A','G','T','C','A'};
    const Bytes A2{'A','G','A','T','C','G','G','A','A','G','A','G','C','G','T','C','G','T','G','T','A','G','G','G','A','A','A','G','A','G','T','G','T'};

    // every shift across the word boundaries: mates and adapters whose X / Y lengths sit at 63, 64, 65, 127, 128, 129 and every fragment length they allow
    int n_pairs = 0;
    for (int la : {0, 1, 31, 33, 63, 64})
        for (int L1 : {1, 30, 31, 32, 33, 63, 64, 65, 95, 96, 97, 128})
            for (int L2 : {1, 31, 32, 33, 64, 65, 127}) {
                const Bytes a1 = bases(la, 0), a2 = bases(la, 0);
                const merge::Rule R = make_rule(a1, a2, 1, 1000, 0, 41, merge::MODE_PAIRS);  // everything with a column is admissible: every candidate's key takes part
                const int F = rnd(0, L1 + L2);
                const Bytes frag = bases(F, 20);
                check_pair(R, sequenced(frag, a1, L1), quals(L1), sequenced(revcomp(frag), a2, L2), quals(L2), a1, a2, "boundaries");
                ++n_pairs;
            }
    // random pairs under the default rule and under random ones
    for (int it = 0; it < 1500; ++it) {
        const bool defaults = it % 2 == 0;
        const Bytes a1 = defaults ? A1 : bases(rnd(0, 64), 0), a2 = defaults ? A2 : bases(rnd(0, 64), 0);
        const merge::Rule R = defaults ? make_rule(a1, a2, 11, 166, 15, 41, merge::MODE_PAIRS)
                                       : make_rule(a1, a2, (uint32_t)rnd(1, 40), (uint32_t)rnd(0, 1000), (uint32_t)rnd(0, 40), (uint32_t)rnd(0, 93), merge::MODE_PAIRS);
        const int big = it % 50 == 0;
        const int L1 = big ? rnd(400, 512) : rnd(1, 160), L2 = big ? rnd(400, 512) : rnd(1, 160);
        const int F = rnd(0, L1 + L2 + 20);
        Bytes frag = bases(F, it % 3 == 0 ? 30 : 0);
        Bytes r1 = sequenced(frag, a1, L1), r2 = sequenced(revcomp(frag), a2, L2);
        if (it % 4 == 1) for (auto& c : r1) if (rnd(0, 99) < 5) c = (uint8_t)"ACGT"[rng() & 3];
        if (it % 7 == 0) { r1 = bases(L1, 10); r2 = bases(L2, 10); }  // nothing in common
        check_pair(R, r1, quals(L1), r2, quals(L2), a1, a2, defaults ? "random, default rule" : "random, random rule");
        ++n_pairs;
    }
    // single-end: X = r1, Y = A1
    for (int it = 0; it < 600; ++it) {
        const Bytes a1 = it % 2 ? A1 : bases(rnd(0, 64), 0), none;
        const merge::Rule R = make_rule(a1, none, (uint32_t)rnd(1, 12), (uint32_t)rnd(0, 300), 15, 41, merge::MODE_SINGLE);
        const int L1 = it % 40 == 0 ? 512 : rnd(1, 200), F = rnd(0, L1 + 10);
        check_pair(R, sequenced(bases(F, 10), a1, L1), quals(L1), none, none, a1, none, "single-end");
        ++n_pairs;
    }
    // the classes decided before any compare
    {
        const merge::Rule R = make_rule(A1, A2, 11, 166, 15, 41, merge::MODE_PAIRS);
        CHECK(merge::early_class(R, 0, 30) == merge::CLS_EMPTY_MATE && merge::early_class(R, 30, 0) == merge::CLS_EMPTY_MATE, "empty mate");
        CHECK(merge::early_class(R, 513, 20) == merge::CLS_TOO_LONG && merge::early_class(R, 20, 513) == merge::CLS_TOO_LONG, "too long");
        CHECK(merge::early_class(R, 0, 600) == merge::CLS_EMPTY_MATE, "empty comes first");
        CHECK(merge::early_class(R, 512, 512) == merge::N_CLASSES, "512 is allowed");
    }
    if (failures) { std::printf("merge selftest: %d failures over %d pairs\n", failures, n_pairs); return 1; }
    std::printf("merge selftest ok: %d pairs\n", n_pairs);
    return 0;
}
