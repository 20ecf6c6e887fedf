// dscore_selftest.cpp — the damage score of mapad_amd/csrc/dscore_core.hpp driven directly on the host: the column rule, the table lookup, the bin rule and the
// rounding rules of host_models.hpp (dscore_quantize, dscore_threshold_q, dscore_table) on hand-made tracks and extreme parameters.  A stand-alone program
// (tests/test_dscore_host.py builds it with -fsanitize=address,undefined and runs it as a child process); exits 0 and prints "dscore selftest ok" when every
// check holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../mapad_amd/csrc/host_models.hpp"
#include "../../mapad_amd/csrc/dscore_core.hpp"

using namespace mapad;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// a table [L][nq] whose every cell names itself: (p * nq + q) * 4 + cell + 1, on the heap so that the sanitizer sees a read beyond it
static std::vector<DscoreRow> naming_table(uint32_t L, uint32_t nq) {
    std::vector<DscoreRow> t((size_t)L * nq);
    for (size_t i = 0; i < t.size(); ++i) for (int c = 0; c < 4; ++c) t[i].v[c] = (int16_t)(i * 4 + c + 1);
    return t;
}
static int32_t score(const std::vector<uint32_t>& ops, const std::string& read, const std::vector<uint8_t>& quals, const std::vector<DscoreRow>& table, uint32_t nq, uint32_t& columns) {
    HitRec h{};
    h.n_ops = (uint32_t)ops.size(); h.ops_off = 0;
    // exact-size heap copies: a load one byte beyond the read or its qualities is an error under the sanitizer
    std::vector<uint8_t> r(read.begin(), read.end());
    return dscore_read(h, ops.data(), r.data(), quals.data(), (uint32_t)r.size(), table.empty() ? nullptr : table.data(), nq, columns);
}

int main() {
    {   // the four cells and nothing else
        const char B[5] = {'A', 'C', 'G', 'T', 'N'};
        int informative = 0;
        for (char r : B) for (char q : B) {
            const uint32_t c = dscore_cell((uint32_t)r, (uint32_t)q);
            informative += c != kDscoreNoCell;
            CHECK((c == DS_CC) == (r == 'C' && q == 'C') && (c == DS_CT) == (r == 'C' && q == 'T') && (c == DS_GG) == (r == 'G' && q == 'G') && (c == DS_GA) == (r == 'G' && q == 'A'));
        }
        CHECK(informative == 4);
    }
    {   // the column rule on a hand-made track, one quality level: read 5' CTGANcg 3'
        const std::string read = "CTGANcg";
        const std::vector<uint8_t> quals = {30, 31, 32, 33, 34, 35, 36};
        const auto T = naming_table(7, 1);
        auto cell_value = [&](uint32_t p, uint32_t c) { return (int32_t)(p * 4 + c + 1); };
        uint32_t cols = 0;
        const std::vector<uint32_t> ops = {
            pack_op(OP_MATCH, 0, 0),         // C = C            -> C->C at 0
            pack_op(OP_MISMATCH, 1, 'C'),    // ref C, read T    -> C->T at 1
            pack_op(OP_INS, 2, 0),           // an insertion of the read's G: nothing
            pack_op(OP_DEL, 2, 'C'),         // a deleted C: nothing
            pack_op(OP_MISMATCH, 3, 'g'),    // ref g (lower case), read A -> G->A at 3
            pack_op(OP_MISMATCH, 4, 'C'),    // read N: nothing
            pack_op(OP_MATCH, 5, 0),         // read c (lower case) = C -> C->C at 5
            pack_op(OP_MATCH, 6, 0),         // read g -> G->G at 6
            pack_op(OP_MATCH, 7, 0),         // p >= L: nothing, and nothing is read
            pack_op(OP_MISMATCH, 0xFFFF, 'C'),
            pack_op(OP_MISMATCH, 2, 'A'),    // ref A, read G: not informative
            pack_op(OP_MISMATCH, 1, 'G'),    // ref G, read T: not informative
        };
        const int32_t s = score(ops, read, quals, T, 1, cols);
        CHECK(cols == 5);
        CHECK(s == cell_value(0, DS_CC) + cell_value(1, DS_CT) + cell_value(3, DS_GA) + cell_value(5, DS_CC) + cell_value(6, DS_GG));
        // the same track in any order gives the same integer
        std::vector<uint32_t> rev(ops.rbegin(), ops.rend());
        uint32_t cols2 = 0;
        CHECK(score(rev, read, quals, T, 1, cols2) == s && cols2 == cols);
        // no table: nothing is informative
        CHECK(score(ops, read, quals, {}, 1, cols2) == 0 && cols2 == 0);
    }
    {   // 256 quality levels: the row is the read's quality byte, 0 and 255 included
        const std::string read = "CG";
        const auto T = naming_table(2, 256);
        uint32_t cols = 0;
        CHECK(score({pack_op(OP_MATCH, 0, 0), pack_op(OP_MATCH, 1, 0)}, read, {0, 255}, T, 256, cols) == (int32_t)(int16_t)((0 * 256 + 0) * 4 + DS_CC + 1) + (int32_t)(int16_t)((1 * 256 + 255) * 4 + DS_GG + 1));
        CHECK(cols == 2);
    }
    {   // L = 1
        const auto T = naming_table(1, 1);
        uint32_t cols = 0;
        CHECK(score({pack_op(OP_MISMATCH, 0, 'C')}, "T", {40}, T, 1, cols) == (int32_t)DS_CT + 1 && cols == 1);
        CHECK(score({pack_op(OP_MATCH, 1, 0)}, "C", {40}, T, 1, cols) == 0 && cols == 0);
        CHECK(score({}, "C", {40}, T, 1, cols) == 0 && cols == 0);
    }
    {   // rounding: ties to even, exact products, saturation
        CHECK(host::dscore_quantize(0.0f) == 0 && host::dscore_quantize(1.0f) == 256 && host::dscore_quantize(-1.0f) == -256);
        CHECK(host::dscore_quantize(0.5f / 256.0f) == 0 && host::dscore_quantize(1.5f / 256.0f) == 2 && host::dscore_quantize(2.5f / 256.0f) == 2 && host::dscore_quantize(-0.5f / 256.0f) == 0);
        CHECK(host::dscore_quantize(-1.5f / 256.0f) == -2);
        CHECK(host::dscore_quantize(127.99f) == 32765 && host::dscore_quantize(128.0f) == 32767 && host::dscore_quantize(1e30f) == 32767);
        CHECK(host::dscore_quantize(-128.0f) == -32768 && host::dscore_quantize(-1e30f) == -32768 && host::dscore_quantize(INFINITY) == 32767 && host::dscore_quantize(-INFINITY) == -32768);
        // an extreme test-model score saturates the table's C->T cell, and only that one
        mapad_params_t p;
        std::memset(&p, 0, sizeof p);
        p.model_kind = MAPAD_MODEL_TEST; p.deam_score = 1000.0f; p.mm_score = -1000.0f; p.match_score = 0.0f;
        std::vector<int16_t> t;
        host::dscore_table(p, 3, host::quality_levels(p), t);
        CHECK(host::quality_levels(p) == 1 && t.size() == 12);
        for (int i = 0; i < 3; ++i) CHECK(t[i * 4 + DS_CC] == 0 && t[i * 4 + DS_CT] == 32767 && t[i * 4 + DS_GG] == 0 && t[i * 4 + DS_GA] == 0);
        p.deam_score = -1000.0f; p.mm_score = 1000.0f;
        t.clear();
        host::dscore_table(p, 1, 1, t);
        CHECK(t[DS_CT] == -32768);
        // saturated cells add as integers: 3 x 32767 does not wrap
        std::vector<DscoreRow> T(3);
        for (auto& row : T) { row.v[0] = 0; row.v[1] = 32767; row.v[2] = 0; row.v[3] = 0; }
        uint32_t cols = 0;
        CHECK(score({pack_op(OP_MISMATCH, 0, 'C'), pack_op(OP_MISMATCH, 1, 'C'), pack_op(OP_MISMATCH, 2, 'C')}, "TTT", {1, 2, 3}, T, 1, cols) == 3 * 32767 && cols == 3);
    }
    {   // the threshold: ceilf at exact and inexact values
        int32_t q = 0;
        CHECK(host::dscore_threshold_q(3.0f, q) && q == 768);
        CHECK(host::dscore_threshold_q(0.0f, q) && q == 0);
        CHECK(host::dscore_threshold_q(0.1f, q) && q == 26);     // 25.6...
        CHECK(host::dscore_threshold_q(-0.1f, q) && q == -25);
        CHECK(host::dscore_threshold_q(1.0f / 256.0f, q) && q == 1);
        CHECK(host::dscore_threshold_q(std::nextafterf(1.0f / 256.0f, 1.0f), q) && q == 2);
        CHECK(host::dscore_threshold_q(1e30f, q) && q == INT32_MAX);
        CHECK(host::dscore_threshold_q(-1e30f, q) && q == INT32_MIN);
        CHECK(!host::dscore_threshold_q(NAN, q));
    }
    {   // the bin rule and what a read adds to an accumulator
        const int32_t at[8] = {-9000, -8192, -1, 0, 127, 128, 8191, 9000};
        const uint32_t bin[8] = {0, 0, 63, 64, 64, 65, 127, 127};
        unsigned long long w[kDscoreWords] = {};
        long long sum = 0;
        for (int k = 0; k < 8; ++k) {
            CHECK(dscore_bin(at[k]) == bin[k]);
            dscore_account(true, at[k], 2, 0, w);
            sum += at[k];
        }
        CHECK(dscore_bin(INT32_MIN) == 0 && dscore_bin(INT32_MAX) == 127 && dscore_bin(-8191) == 0 && dscore_bin(-8064) == 1 && dscore_bin(-128) == 63 && dscore_bin(8063) == 126 && dscore_bin(8064) == 127);
        dscore_account(false, 0, 0, 0, w);  // an unscored read: seen, nothing else
        CHECK(w[DS_READS_SEEN] == 9 && w[DS_READS_SCORED] == 8 && w[DS_READS_BELOW] == 3 && w[DS_COLUMNS] == 16 && (long long)w[DS_SCORE_SUM] == sum);
        CHECK(w[DS_SCALARS + 0] == 2 && w[DS_SCALARS + 63] == 1 && w[DS_SCALARS + 64] == 2 && w[DS_SCALARS + 65] == 1 && w[DS_SCALARS + 127] == 2);
        unsigned long long total = 0;
        for (uint32_t k = 0; k < kDscoreBins; ++k) total += w[DS_SCALARS + k];
        CHECK(total == 8);
        // a negative sum survives the unsigned accumulator
        unsigned long long n[kDscoreWords] = {};
        dscore_account(true, -5, 1, -4, n);
        dscore_account(true, -7, 1, -4, n);
        CHECK((long long)n[DS_SCORE_SUM] == -12 && n[DS_READS_BELOW] == 2);
    }
    std::printf("dscore selftest ok\n");
    return 0;
}
