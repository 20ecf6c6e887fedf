// genotype_selftest.cpp — the diploid genotype likelihoods of mapad_amd/csrc/genotype_core.hpp driven directly on the host: the pair table's rounding, the
// strand map, the call rule, GQ / PL and the text's end, on hand-made tables and tracks.  A stand-alone program (tests/test_genotype_host.py builds it with
// -fsanitize=address,undefined and runs it as a child process); exits 0 and prints "genotype selftest ok" when every check holds.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../mapad_amd/csrc/host_models.hpp"
#include "../../mapad_amd/csrc/genotype_core.hpp"

using namespace mapad;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// A table for one read length [L][nq][4 read bases] of rows whose every value names itself: value_q(p, q, to, pair), on the heap at its exact size so that the
// sanitizer sees a read beyond it (operator new aligns to 16 bytes: a row is one aligned load).
static int16_t value_q(uint32_t nq, uint32_t p, uint32_t q, uint32_t to, uint32_t pair) { return (int16_t)(-(int32_t)((((p * nq + q) * 4 + to) * 6 + pair) % 30000) - 1); }
struct Table {
    std::vector<GenotypeRow> rows;
    uint32_t nq;
    Table(uint32_t L, uint32_t nq_) : rows((size_t)L * nq_ * 4), nq(nq_) {
        for (uint32_t p = 0; p < L; ++p) for (uint32_t q = 0; q < nq; ++q) for (uint32_t to = 0; to < 4; ++to) {
            GenotypeRow& r = rows[((size_t)p * nq + q) * 4 + to];
            for (uint32_t k = 0; k < 6; ++k) r.v[k] = value_q(nq, p, q, to, k);
            r.v[6] = r.v[7] = 0;
        }
    }
};
struct Acc {
    uint64_t S;
    std::vector<int32_t> het;
    uint64_t columns = 0;
    explicit Acc(uint64_t s) : S(s), het(s * 6, 0) {}
    bool untouched() const { for (int32_t v : het) if (v) return false; return columns == 0; }
};
static bool add(Acc& A, const Table& T, int32_t base, const std::vector<uint32_t>& ops, const std::string& read, const std::vector<uint8_t>& quals, uint64_t abs, bool backward,
                PileupFilter F = PileupFilter{0, 0, 0}, int mode = 1, uint64_t x0 = 1, bool skip = false) {
    HitRec h{};
    h.n_ops = (uint32_t)ops.size(); h.ops_off = 0;
    CoordRec cr{};
    cr.mapped = 1; cr.error = 0; cr.x0 = x0; cr.best = 0; cr.first.abs = abs; cr.first.backward = backward ? 1 : 0;
    std::vector<uint8_t> r(read.begin(), read.end());  // exact-size heap copies
    return genotype_read(cr, &h, ops.data(), r.data(), quals.data(), (uint32_t)r.size(), mode, F, T.rows.data(), base, T.nq, A.S, A.het.data(), &A.columns, skip);
}
static uint32_t call_of(const int32_t (&ll)[4], const int32_t (&het)[6], uint32_t depth, uint32_t min_depth, int32_t mq, int32_t pq, int64_t& m, int64_t* g_out = nullptr, int64_t* best_out = nullptr) {
    int64_t g[GT_COUNT], best;
    const uint32_t c = genotype_call(ll, het, depth, min_depth, mq, pq, g, best, m);
    if (g_out) std::memcpy(g_out, g, sizeof g);
    if (best_out) *best_out = best;
    return c;
}

int main() {
    {   // the genotypes' alleles and the strand map: complementing both alleles of a pair
        static const uint32_t X[10] = {0, 1, 2, 3, 0, 0, 0, 1, 1, 2}, Y[10] = {0, 1, 2, 3, 1, 2, 3, 2, 3, 3};
        for (uint32_t g = 0; g < GT_COUNT; ++g) CHECK(genotype_allele(g, 0) == X[g] && genotype_allele(g, 1) == Y[g]);
        for (uint32_t k = 0; k < 6; ++k) {
            const uint32_t x = 3 - Y[4 + k], y = 3 - X[4 + k];  // the complements, in order again
            const uint32_t m = genotype_strand_pair(k);
            CHECK(X[4 + m] == x && Y[4 + m] == y && genotype_strand_pair(m) == k);
        }
        CHECK(genotype_strand_pair(0) == 5 && genotype_strand_pair(1) == 4 && genotype_strand_pair(2) == 2 && genotype_strand_pair(3) == 3);
        GenotypeRow r{{10, 11, 12, 13, 14, 15, 0, 0}};
        int32_t v[6];
        genotype_column_values(r, false, v);
        for (uint32_t k = 0; k < 6; ++k) CHECK(v[k] == 10 + (int32_t)k);
        genotype_column_values(r, true, v);
        for (uint32_t k = 0; k < 6; ++k) CHECK(v[k] == 10 + (int32_t)genotype_strand_pair(k));
        CHECK(sizeof(GenotypeRow) == 16 && alignof(GenotypeRow) == 16);
    }
    {   // the pair value: between its two alleles' values, never more than one bit below the larger; equal alleles give the allele; nothing or a NaN: the lower end
        CHECK(host::genotype_pair_quantized(-1.0f, -1.0f) == -256);
        CHECK(host::genotype_pair_quantized(0.0f, -200.0f) == -256);            // log2(0.5)
        CHECK(host::genotype_pair_quantized(-200.0f, 0.0f) == -256);
        CHECK(host::genotype_pair_quantized(-2.0f, -3.0f) == host::dscore_quantize((float)std::log2(0.5 * 0.25 + 0.5 * 0.125)));
        const float inf = std::numeric_limits<float>::infinity();
        CHECK(host::genotype_pair_quantized(-inf, -inf) == -32768 && host::genotype_pair_quantized(std::numeric_limits<float>::quiet_NaN(), -1.0f) == -32768);
        CHECK(host::genotype_pair_quantized(-inf, -1.0f) == -512 && host::genotype_pair_quantized(-2000.0f, -2000.0f) == -32768);
        for (int a = -3000; a <= 0; a += 37) for (int b = -3000; b <= 0; b += 53) {
            const float sa = (float)a / 100.0f, sb = (float)b / 100.0f;
            const int32_t h = host::genotype_pair_quantized(sa, sb), qa = host::dscore_quantize(sa), qb = host::dscore_quantize(sb);
            CHECK(h >= std::min(qa, qb) - 1 && h <= std::max(qa, qb) + 1 && h >= std::max(qa, qb) - 256 - 1);
        }
    }
    {   // the table: [len][nq][4][8], six pair values then two zero words; the test model's flat scores
        mapad_params_t p{};
        p.model_kind = MAPAD_MODEL_TEST; p.deam_score = -0.5f; p.mm_score = -1.0f; p.match_score = 0.0f;
        std::vector<GenotypeRow> t;
        host::genotype_table(p, 3, 1, t);
        CHECK(t.size() == 3 * 4);
        for (const GenotypeRow& r : t) CHECK(r.v[6] == 0 && r.v[7] == 0);
        // read base T: under C/T half deaminated (log2(0.5 * 2^-0.5 + 0.5) rounded), under A/T half a mismatch; the same at every position of this model
        CHECK(t[3].v[4] == host::genotype_pair_quantized(-0.5f, 0.0f) && t[3].v[2] == host::genotype_pair_quantized(-1.0f, 0.0f) && t[4 + 3].v[4] == t[3].v[4] && t[8 + 3].v[2] == t[3].v[2]);
        host::genotype_table(p, 2, 1, t);  // appended behind
        CHECK(t.size() == (3 + 2) * 4);
        for (uint32_t x = 0; x < 4; ++x) for (uint32_t y = x + 1; y < 4; ++y) { const uint32_t g = genotype_of_pair(x, y); CHECK(g >= 4 && g < GT_COUNT && genotype_allele(g, 0) == x && genotype_allele(g, 1) == y); }
    }
    {   // the call rule
        int64_t m = -1, g[GT_COUNT], best = 0;
        const int32_t z4[4] = {0, 0, 0, 0}, z6[6] = {0, 0, 0, 0, 0, 0};
        CHECK(call_of(z4, z6, 0, 1, 1, 0, m) == kGenotypeNoCall && m == 0);                                         // nothing contributed
        const int32_t hom[4] = {-10, -800, -900, -1000}, hets[6] = {-300, -400, -500, -2000, -2000, -2000};
        CHECK(call_of(hom, hets, 3, 1, 256, 0, m, g, &best) == GT_AA && m == 290 && best == -10 && g[GT_AC] == -300 && genotype_quality(GT_AA, m) == 3);
        CHECK(call_of(hom, hets, 3, 1, 291, 0, m) == kGenotypeNoCall && m == 290 && genotype_quality(kGenotypeNoCall, m) == 0);  // one unit short
        CHECK(call_of(hom, hets, 3, 4, 256, 0, m) == kGenotypeNoCall);                                              // too shallow
        CHECK(call_of(hom, hets, 3, 1, 256, 1000, m, g) == GT_AA && m == 790 && g[GT_AC] == -1300);                 // the penalty lowers the hets only
        const int32_t het_best[6] = {-5, -400, -500, -2000, -2000, -2000};
        CHECK(call_of(hom, het_best, 3, 1, 1, 0, m) == GT_AC && m == 5);                                            // a het leads
        CHECK(call_of(hom, het_best, 3, 1, 1, 5, m) == kGenotypeNoCall && m == 0);                                  // the penalty makes a tie: first in order, margin 0
        CHECK(call_of(hom, het_best, 3, 1, 1, 6, m) == GT_AA && m == 1);                                            // ... and flips the het to the hom
        const int32_t tie4[4] = {-7, -7, -900, -900};
        CHECK(call_of(tie4, hets, 2, 1, 1, 0, m) == kGenotypeNoCall && m == 0);                                     // two equal maxima
        const int32_t tie6[6] = {-3, -3, -9, -9, -9, -9};
        int64_t gg[GT_COUNT], bb;
        const int32_t low4[4] = {-50, -50, -50, -50};
        CHECK(genotype_call(low4, tie6, 2, 1, 0, 0, gg, bb, m) == GT_AC && m == 0 && bb == -3);                     // (a rule of margin 0, never from the library: the FIRST maximum)
        // int64 margins near +-2^31: the cells' whole range, and the penalty on top
        const int32_t top[4] = {INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN}, bottom[6] = {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
        CHECK(call_of(top, bottom, 1, 1, INT32_MAX, 0, m) == GT_AA && m == 4294967295ll && genotype_quality(GT_AA, m) == 99);
        CHECK(call_of(top, bottom, 1, 1, INT32_MAX, INT32_MAX, m, g, &best) == GT_AA && m == 4294967295ll && g[GT_GT] == (int64_t)INT32_MIN - INT32_MAX && genotype_pl(best, g[GT_GT]) == 255);
        const int32_t all_min[4] = {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN}, one_up[6] = {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN + 1};
        CHECK(call_of(all_min, one_up, 1, 1, 1, 0, m) == GT_GT && m == 1);
        CHECK(call_of(all_min, one_up, 1, 1, 1, 1, m) == kGenotypeNoCall && m == 0);
        CHECK(call_of(all_min, one_up, 1, 1, 1, 2, m) == kGenotypeNoCall && m == 0);                                // (four equal homs lead: margin 0)
        const int32_t hi6[6] = {INT32_MAX, 0, 0, 0, 0, 0};
        CHECK(call_of(all_min, hi6, 1, 1, 1, 0, m) == GT_AC && m == 2147483647ll);
        // GQ and PL: 301 / 25600 per unit, integer division, clamps
        CHECK(genotype_quality(GT_CC, 0) == 0 && genotype_quality(GT_CC, 85) == 0 && genotype_quality(GT_CC, 86) == 1 && genotype_quality(GT_CC, 768) == 9 &&
              genotype_quality(GT_CC, 8419) == 98 && genotype_quality(GT_CC, 8420) == 99 && genotype_quality(GT_CC, 1ll << 33) == 99);
        CHECK(genotype_pl(-10, -10) == 0 && genotype_pl(-10, -95) == 0 && genotype_pl(-10, -96) == 1 && genotype_pl(0, -21687) == 254 && genotype_pl(0, -21688) == 255 &&
              genotype_pl(INT32_MAX, (int64_t)INT32_MIN - INT32_MAX) == 255);
        unsigned long long w[GTC_WORDS] = {};
        CHECK(genotype_site(hom, hets, 2, 2, 256, 0, w, m) == GT_AA && genotype_site(hom, het_best, 7, 2, 1, 0, w, m) == GT_AC && genotype_site(z4, z6, 0, 2, 1, 0, w, m) == kGenotypeNoCall);
        CHECK(genotype_site(hom, hets, 1, 2, 256, 0, w, m) == kGenotypeNoCall);
        CHECK(w[GTC_COVERED] == 3 && w[GTC_DEEP] == 2 && w[GTC_CALLED] == 2 && w[GTC_CALLED_GT + GT_AA] == 1 && w[GTC_CALLED_GT + GT_AC] == 1 && w[GTC_CALLED_GT + GT_CC] == 0 &&
              w[GTC_MAX_DEPTH] == 7 && w[GTC_MARGIN_SUM] == 295);
    }
    {   // a forward read and the same read backward: a backward column adds the row under the strand map; one quality level and 256 levels
        for (uint32_t nq : {1u, 256u}) {
            const Table T(4, nq);
            const std::string read = "ACGT";
            const std::vector<uint8_t> quals = {30, 2, 255, 0};
            const std::vector<uint32_t> fwd = {pack_op(OP_MATCH, 0, 0), pack_op(OP_MISMATCH, 1, 'A'), pack_op(OP_MATCH, 2, 0), pack_op(OP_MATCH, 3, 0)};
            Acc F(10), B(10);
            CHECK(add(F, T, 0, fwd, read, quals, 3, false));
            CHECK(add(B, T, 0, fwd, read, quals, 3, true));
            for (uint32_t p = 0; p < 4; ++p) {
                const uint32_t q = nq == 1 ? 0 : quals[p], to = p;  // the read's p-th base is base p
                for (uint32_t k = 0; k < 6; ++k) {
                    CHECK(F.het[(3 + p) * 6 + k] == value_q(nq, p, q, to, k));
                    CHECK(B.het[(3 + (3 - p)) * 6 + k] == value_q(nq, p, q, to, genotype_strand_pair(k)));  // read position p lies at reference offset 3 - p
                }
            }
            CHECK(F.columns == 4 && B.columns == 4);
            for (uint64_t x : {0ull, 1ull, 2ull, 7ull, 8ull, 9ull}) for (int k = 0; k < 6; ++k) CHECK(F.het[x * 6 + k] == 0 && B.het[x * 6 + k] == 0);
        }
    }
    {   // insertions, deletions, N, lower case, masks, the quality floor, p >= L, mode 2, skip: the columns allele_read counts
        const Table T(7, 256);
        const std::string read = "CtGANcg";
        const std::vector<uint8_t> quals = {30, 31, 32, 33, 34, 35, 36};
        const std::vector<uint32_t> ops = {pack_op(OP_MATCH, 0, 0), pack_op(OP_MISMATCH, 1, 'C'), pack_op(OP_INS, 2, 0), pack_op(OP_DEL, 2, 'C'), pack_op(OP_MATCH, 3, 0),
                                           pack_op(OP_MISMATCH, 4, 'C'), pack_op(OP_MATCH, 5, 0), pack_op(OP_MATCH, 6, 0), pack_op(OP_MATCH, 9, 0)};
        Acc A(20);
        CHECK(add(A, T, 0, ops, read, quals, 5, false));
        const uint32_t at[7] = {5, 6, 0, 8, 9, 10, 11}, to[7] = {1, 3, 2, 0, 4, 1, 2};
        for (uint32_t p : {0u, 1u, 3u, 5u, 6u}) for (uint32_t k = 0; k < 6; ++k) CHECK(A.het[at[p] * 6 + k] == value_q(256, p, quals[p], to[p], k));
        for (uint64_t x : {7ull, 9ull, 12ull}) for (int k = 0; k < 6; ++k) CHECK(A.het[x * 6 + k] == 0);
        CHECK(A.columns == 5);
        Acc M(20);
        CHECK(add(M, T, 0, ops, read, quals, 5, false, PileupFilter{32, 1, 1}) && M.columns == 2 && M.het[5 * 6] == 0 && M.het[6 * 6] == 0 && M.het[8 * 6] != 0 && M.het[10 * 6] != 0 && M.het[11 * 6] == 0);
        Acc U(20);
        CHECK(add(U, T, 0, ops, read, quals, 5, false, PileupFilter{0, 0, 0}, 2, 2) && U.untouched());        // mode 2, X0 = 2
        CHECK(add(U, T, 0, ops, read, quals, 5, false, PileupFilter{0, 0, 0}, 2, 1, true) && U.untouched());  // skipped
        CHECK(add(U, T, 0, ops, read, quals, 5, false, PileupFilter{0, 0, 0}, 2, 1) && U.columns == 5);
    }
    {   // the text's end: a read ending on the last position is written, one position further is reported and writes nothing; so does a missing table
        const Table T(3, 1);
        const std::string read = "GAT";
        const std::vector<uint8_t> quals = {40, 40, 40};
        const std::vector<uint32_t> ops = {pack_op(OP_MATCH, 0, 0), pack_op(OP_MATCH, 1, 0), pack_op(OP_MATCH, 2, 0)};
        for (bool backward : {false, true}) {
            Acc A(8);
            CHECK(add(A, T, 0, ops, read, quals, 5, backward) && A.columns == 3 && A.het[7 * 6 + 5] != 0 && A.het[4 * 6] == 0);
            Acc X(8);
            CHECK(!add(X, T, 0, ops, read, quals, 6, backward) && X.untouched());
            CHECK(!add(X, T, 0, ops, read, quals, 9, backward) && X.untouched());
            CHECK(!add(X, T, 0, ops, read, quals, ~0ull, backward) && X.untouched());
        }
        const std::vector<uint32_t> with_del = {pack_op(OP_MATCH, 0, 0), pack_op(OP_DEL, 1, 'A'), pack_op(OP_MATCH, 1, 0), pack_op(OP_MATCH, 2, 0)};
        Acc D(8);
        CHECK(add(D, T, 0, with_del, read, quals, 4, false) && D.het[4 * 6] != 0 && D.het[5 * 6] == 0 && D.het[6 * 6] != 0 && D.het[7 * 6] != 0);
        CHECK(!add(D, T, 0, with_del, read, quals, 5, false));
        Acc N(8);
        CHECK(!add(N, T, -1, ops, read, quals, 0, false) && N.untouched());  // no table for this length
    }
    {   // sums wrap like the device's atomic add instead of overflowing
        const Table T(1, 1);
        Acc A(2);
        A.het[0] = INT32_MIN - (int32_t)value_q(1, 0, 0, 0, 0) - 1;  // one unit short of wrapping under AC
        CHECK(add(A, T, 0, {pack_op(OP_MATCH, 0, 0)}, "A", {10}, 0, false));
        CHECK(A.het[0] == INT32_MAX);
    }
    std::printf("genotype selftest ok\n");
    return 0;
}
