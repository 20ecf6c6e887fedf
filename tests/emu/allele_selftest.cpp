// allele_selftest.cpp — the allele likelihoods of mapad_amd/csrc/allele_core.hpp driven directly on the host: the rounding rule, the call rule, the strand
// flip and the text's end, on hand-made tables and tracks.  A stand-alone program (tests/test_allele_host.py builds it with -fsanitize=address,undefined and
// runs it as a child process); exits 0 and prints "allele selftest ok" when every check holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../mapad_amd/csrc/host_models.hpp"
#include "../../mapad_amd/csrc/allele_core.hpp"

using namespace mapad;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// A table for one read length [L][nq][5 read bases][4 true bases] whose every value names itself in units: value_q(p, q, to, from) / 256, on the heap at its
// exact size so that the sanitizer sees a read beyond it.  Distinct small integers: every one survives the rounding unchanged.
static int32_t value_q(uint32_t nq, uint32_t p, uint32_t q, uint32_t to, uint32_t from) { return -(int32_t)((((p * nq + q) * 5 + to) * 4 + from) % 30000) - 1; }
struct Tables {
    std::vector<float> sdm;
    std::vector<int32_t> base;
    DevParams P{};
    Tables(uint32_t L, uint32_t nq) : sdm((size_t)L * nq * 5 * 4), base(kMaxReadLen + 1, -1) {
        for (uint32_t p = 0; p < L; ++p) for (uint32_t q = 0; q < nq; ++q) for (uint32_t to = 0; to < 5; ++to) for (uint32_t f = 0; f < 4; ++f)
            sdm[(((size_t)p * nq + q) * 5 + to) * 4 + f] = (float)value_q(nq, p, q, to, f) / 256.0f;
        base[L] = 0;
        P.sdm_table = sdm.data(); P.table_base = base.data(); P.nq = (int32_t)nq;
    }
};
struct Acc {
    uint64_t S;
    std::vector<int32_t> ll;
    std::vector<uint32_t> depth;
    unsigned long long scalars[AL_SCALARS] = {};
    explicit Acc(uint64_t s) : S(s), ll(s * 4, 0), depth(s, 0) {}
    bool untouched() const { for (int32_t v : ll) if (v) return false; for (uint32_t v : depth) if (v) return false; return true; }
};
// one mapped read with the given track at absolute position abs
static bool add(Acc& A, const Tables& T, const std::vector<uint32_t>& ops, const std::string& read, const std::vector<uint8_t>& quals, uint64_t abs, bool backward,
                PileupFilter F = PileupFilter{0, 0, 0}, int mode = 1, uint64_t x0 = 1, bool skip = false) {
    HitRec h{};
    h.n_ops = (uint32_t)ops.size(); h.ops_off = 0;
    CoordRec cr{};
    cr.mapped = 1; cr.error = 0; cr.x0 = x0; cr.best = 0; cr.first.abs = abs; cr.first.backward = backward ? 1 : 0;
    std::vector<uint8_t> r(read.begin(), read.end());  // exact-size heap copies
    const uint32_t L = (uint32_t)r.size();
    return allele_read(cr, &h, ops.data(), r.data(), quals.data(), L, mode, F, T.P, T.P.table_base[L], A.S, A.ll.data(), A.depth.data(), A.scalars, skip);
}
static int32_t reference_quantize(float v) {  // saturate_i16(rintf(v * 256)), written the way host::dscore_quantize writes it
    return (int32_t)host::dscore_quantize(v);
}

int main() {
    {   // allele_quantize: ties to even, saturation, -0, and agreement with the damage score's rule over a sweep
        CHECK(allele_quantize(0.5f / 256.0f) == 0 && allele_quantize(1.5f / 256.0f) == 2 && allele_quantize(2.5f / 256.0f) == 2 && allele_quantize(-0.5f / 256.0f) == 0);
        CHECK(allele_quantize(-1.5f / 256.0f) == -2 && allele_quantize(-2.5f / 256.0f) == -2 && allele_quantize(3.5f / 256.0f) == 4);
        CHECK(allele_quantize(-0.0f) == 0 && allele_quantize(0.0f) == 0);
        CHECK(allele_quantize(128.0f) == 32767 && allele_quantize(1e30f) == 32767 && allele_quantize(std::numeric_limits<float>::infinity()) == 32767);
        CHECK(allele_quantize(-128.0f) == -32768 && allele_quantize(-128.5f) == -32768 && allele_quantize(-1e30f) == -32768);
        CHECK(allele_quantize(-std::numeric_limits<float>::infinity()) == -32768 && allele_quantize(std::numeric_limits<float>::quiet_NaN()) == -32768);
        CHECK(allele_quantize(32766.5f / 256.0f) == 32766 && allele_quantize(32766.75f / 256.0f) == 32767 && allele_quantize(-32767.5f / 256.0f) == -32768);
        for (int k = -70000; k <= 70000; ++k) {
            const float v = (float)k / 512.0f;  // every half unit across and beyond the int16 range
            CHECK(allele_quantize(v) == reference_quantize(v));
            const float w = std::nextafter(v, 1e9f);
            CHECK(allele_quantize(w) == reference_quantize(w));
        }
    }
    {   // the smallest margin: at least one unit, ceilf, not a number refused
        int32_t q = 0;
        CHECK(host::allele_min_margin_q(3.0f, q) && q == 768);
        CHECK(host::allele_min_margin_q(0.0f, q) && q == 1);
        CHECK(host::allele_min_margin_q(-5.0f, q) && q == 1);
        CHECK(host::allele_min_margin_q(0.1f, q) && q == 26);
        CHECK(host::allele_min_margin_q(1e30f, q) && q == INT32_MAX);
        CHECK(!host::allele_min_margin_q(std::numeric_limits<float>::quiet_NaN(), q));
    }
    {   // the call rule
        int64_t m = -1;
        CHECK(allele_call(0, 0, 0, 0, 0, 1, 1, m) == kPileupNoCall && m == 0);                       // nothing contributed
        CHECK(allele_call(-5, -5, -900, -900, 2, 1, 1, m) == kPileupNoCall && m == 0);                // two equal maxima: margin 0
        CHECK(allele_call(-900, -5, -5, -900, 2, 1, 1, m) == kPileupNoCall && m == 0);
        CHECK(allele_call(-7, -7, -7, -7, 3, 1, 1, m) == kPileupNoCall && m == 0);                    // four equal cells
        CHECK(allele_call(-10, -800, -900, -1000, 1, 1, 768, m) == 0 && m == 790 && allele_quality(0, m) == 3);
        CHECK(allele_call(-1000, -800, -900, -10, 1, 1, 768, m) == 3 && m == 790);
        CHECK(allele_call(-1000, -10, -777, -800, 1, 1, 768, m) == kPileupNoCall && m == 767);       // one unit short
        CHECK(allele_call(-1000, -10, -778, -800, 1, 1, 768, m) == 1 && m == 768);                    // exactly the margin
        CHECK(allele_call(-1000, -10, -778, -800, 1, 2, 768, m) == kPileupNoCall && m == 768);        // too shallow
        CHECK(allele_call(5, -1, -1, -1, 1, 1, 1, m) == 0 && m == 6);                                 // a single positive cell (a model may score above 0)
        CHECK(allele_call(-3, -2, -1, -4, 1, 1, 1, m) == 2 && m == 1);                                // all negative
        CHECK(allele_call(INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN, 1, 1, INT32_MAX, m) == 0 && m == 4294967295ll && allele_quality(0, m) == 255);  // beyond int32
        CHECK(allele_call(INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN + 1, 1, 1, 1, m) == 3 && m == 1);
        CHECK(allele_call(INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN, 9, 1, 1, m) == kPileupNoCall && m == 0);
        CHECK(allele_call(0, INT32_MAX, INT32_MAX - 1, 0, 1, 1, 2, m) == kPileupNoCall && m == 1);
        CHECK(allele_quality(kPileupNoCall, 99999) == 0 && allele_quality(2, 255) == 0 && allele_quality(2, 256) == 1 && allele_quality(2, 65535) == 255 &&
              allele_quality(2, 65536) == 255 && allele_quality(2, 65279) == 254);
        unsigned long long w[ALC_WORDS] = {};
        const int32_t a[4] = {-10, -800, -900, -1000}, b[4] = {-5, -5, -9, -9}, z[4] = {0, 0, 0, 0};
        CHECK(allele_site(a, 2, 2, 768, w, m) == 0 && allele_site(b, 7, 2, 768, w, m) == kPileupNoCall && allele_site(z, 0, 2, 768, w, m) == kPileupNoCall);
        CHECK(allele_site(a, 1, 2, 768, w, m) == kPileupNoCall);
        CHECK(w[ALC_COVERED] == 3 && w[ALC_DEEP] == 2 && w[ALC_CALLED] == 1 && w[ALC_CALLED_BASE] == 1 && w[ALC_CALLED_BASE + 1] == 0 && w[ALC_MAX_DEPTH] == 7 &&
              w[ALC_MARGIN_SUM] == 790);
    }
    {   // a forward read and the same read backward: the cell of a backward column is the row reversed; one quality level and 256 levels
        for (uint32_t nq : {1u, 256u}) {
            const Tables T(4, nq);
            const std::string read = "ACGT";
            const std::vector<uint8_t> quals = {30, 2, 255, 0};
            const std::vector<uint32_t> fwd = {pack_op(OP_MATCH, 0, 0), pack_op(OP_MISMATCH, 1, 'A'), pack_op(OP_MATCH, 2, 0), pack_op(OP_MATCH, 3, 0)};
            Acc F(10), B(10);
            CHECK(add(F, T, fwd, read, quals, 3, false));
            // the backward record's track is in read order, its reference order the reverse (coverage_ref_op)
            CHECK(add(B, T, fwd, read, quals, 3, true));
            for (uint32_t p = 0; p < 4; ++p) {
                const uint32_t q = nq == 1 ? 0 : quals[p], to = p;  // the read's p-th base is base p
                for (uint32_t a = 0; a < 4; ++a) {
                    CHECK(F.ll[(3 + p) * 4 + a] == value_q(nq, p, q, to, a));
                    CHECK(B.ll[(3 + (3 - p)) * 4 + a] == value_q(nq, p, q, to, 3 - a));  // read position p lies at reference offset 3 - p; allele a is true base 3 - a
                }
                CHECK(F.depth[3 + p] == 1 && B.depth[3 + p] == 1);
            }
            CHECK(F.scalars[AL_COUNTED] == 4 && F.scalars[AL_READS] == 1 && F.scalars[AL_READS_SEEN] == 1 && B.scalars[AL_COUNTED] == 4);
            for (uint64_t x : {0ull, 1ull, 2ull, 7ull, 8ull, 9ull}) for (int a = 0; a < 4; ++a) CHECK(F.ll[x * 4 + a] == 0 && B.ll[x * 4 + a] == 0 && F.depth[x] == 0);
        }
    }
    {   // insertions, deletions, N, lower case, masks, the quality floor, p >= L, mode 2, skip
        const Tables T(7, 256);
        const std::string read = "CtGANcg";
        const std::vector<uint8_t> quals = {30, 31, 32, 33, 34, 35, 36};
        const std::vector<uint32_t> ops = {pack_op(OP_MATCH, 0, 0), pack_op(OP_MISMATCH, 1, 'C'), pack_op(OP_INS, 2, 0), pack_op(OP_DEL, 2, 'C'), pack_op(OP_MATCH, 3, 0),
                                           pack_op(OP_MISMATCH, 4, 'C'), pack_op(OP_MATCH, 5, 0), pack_op(OP_MATCH, 6, 0), pack_op(OP_MATCH, 9, 0)};
        Acc A(20);
        CHECK(add(A, T, ops, read, quals, 5, false));
        // offsets: p0 -> 5, p1 -> 6, (ins), del -> 7, p3 -> 8, p4 (N) -> 9, p5 -> 10, p6 -> 11, p = 9 >= L -> 12
        const uint32_t at[7] = {5, 6, 0, 8, 9, 10, 11}, to[7] = {1, 3, 2, 0, 4, 1, 2};
        for (uint32_t p : {0u, 1u, 3u, 5u, 6u}) { for (uint32_t a = 0; a < 4; ++a) CHECK(A.ll[at[p] * 4 + a] == value_q(256, p, quals[p], to[p], a)); CHECK(A.depth[at[p]] == 1); }
        for (uint64_t x : {7ull, 9ull, 12ull}) { CHECK(A.depth[x] == 0); for (int a = 0; a < 4; ++a) CHECK(A.ll[x * 4 + a] == 0); }
        CHECK(A.scalars[AL_COUNTED] == 5 && A.scalars[AL_NOT_ACGT] == 2 && A.scalars[AL_INS] == 1 && A.scalars[AL_DELETED] == 1 && A.scalars[AL_MASKED] == 0);
        Acc M(20);
        CHECK(add(M, T, ops, read, quals, 5, false, PileupFilter{32, 1, 1}));
        CHECK(M.scalars[AL_MASKED] == 2 && M.scalars[AL_LOW_QUAL] == 1 && M.scalars[AL_COUNTED] == 2 && M.scalars[AL_NOT_ACGT] == 2);  // p0, p6 masked; p1 (Q31) low
        CHECK(M.depth[5] == 0 && M.depth[6] == 0 && M.depth[8] == 1 && M.depth[10] == 1 && M.depth[11] == 0);
        Acc W(20);  // a read of at most mask5 + mask3 bases: masked entirely, still a read
        CHECK(add(W, T, ops, read, quals, 5, false, PileupFilter{0, 4, 3}) && W.untouched() && W.scalars[AL_READS] == 1 && W.scalars[AL_MASKED] == 5);
        Acc U(20);
        CHECK(add(U, T, ops, read, quals, 5, false, PileupFilter{0, 0, 0}, 2, 2) && U.untouched() && U.scalars[AL_READS] == 0 && U.scalars[AL_READS_SEEN] == 1);  // mode 2, X0 = 2
        CHECK(add(U, T, ops, read, quals, 5, false, PileupFilter{0, 0, 0}, 2, 1, true) && U.untouched() && U.scalars[AL_READS_SEEN] == 2);                          // skipped
        CHECK(add(U, T, ops, read, quals, 5, false, PileupFilter{0, 0, 0}, 2, 1) && U.scalars[AL_READS] == 1 && U.scalars[AL_COUNTED] == 5);
    }
    {   // the text's end: a read ending on the last position is written, one position further raises the flag and writes nothing; so does a missing table
        const Tables T(3, 1);
        const std::string read = "GAT";
        const std::vector<uint8_t> quals = {40, 40, 40};
        const std::vector<uint32_t> ops = {pack_op(OP_MATCH, 0, 0), pack_op(OP_MATCH, 1, 0), pack_op(OP_MATCH, 2, 0)};
        for (bool backward : {false, true}) {
            Acc A(8);
            CHECK(add(A, T, ops, read, quals, 5, backward));
            CHECK(A.depth[5] == 1 && A.depth[6] == 1 && A.depth[7] == 1 && A.depth[4] == 0 && A.scalars[AL_COUNTED] == 3);
            Acc X(8);
            CHECK(!add(X, T, ops, read, quals, 6, backward) && X.untouched() && X.scalars[AL_READS] == 0 && X.scalars[AL_COUNTED] == 0);
            CHECK(!add(X, T, ops, read, quals, 9, backward) && X.untouched());
            CHECK(!add(X, T, ops, read, quals, ~0ull, backward) && X.untouched());
        }
        const std::vector<uint32_t> with_del = {pack_op(OP_MATCH, 0, 0), pack_op(OP_DEL, 1, 'A'), pack_op(OP_MATCH, 1, 0), pack_op(OP_MATCH, 2, 0)};
        Acc D(8);
        CHECK(add(D, T, with_del, read, quals, 4, false) && D.depth[4] == 1 && D.depth[5] == 0 && D.depth[6] == 1 && D.depth[7] == 1);
        CHECK(!add(D, T, with_del, read, quals, 5, false));
        const Tables Other(4, 1);  // no table for a read of 3 bases
        Acc N(8);
        CHECK(!add(N, Other, ops, read, quals, 0, false) && N.untouched());
    }
    {   // sums wrap like the device's atomic add instead of overflowing
        const Tables T(1, 1);
        Acc A(2);
        A.ll[0] = INT32_MIN - value_q(1, 0, 0, 0, 0) - 1;  // one unit short of wrapping under allele A
        CHECK(add(A, T, {pack_op(OP_MATCH, 0, 0)}, "A", {10}, 0, false));
        CHECK(A.ll[0] == INT32_MAX);
    }
    std::printf("allele selftest ok\n");
    return 0;
}
