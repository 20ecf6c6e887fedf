// rescale_selftest.cpp — the quality rescaling of mapad_amd/csrc/rescale_core.hpp driven directly on the host: the column rule, the table lookup, what a read
// writes and counts, and the table rule of host_models.hpp (sdm_prob, rescale_quality, rescale_table) on hand-made tracks and extreme parameters.  A stand-alone
// program (tests/test_rescale_host.py builds it with -fsanitize=address,undefined and runs it as a child process); exits 0 and prints "rescale selftest ok" when
// every check holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../mapad_amd/csrc/host_models.hpp"
#include "../../mapad_amd/csrc/rescale_core.hpp"

using namespace mapad;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// a table [L][256][2] that halves every quality (C->T) or takes 3 off it, floored at 0 (G->A); the row of 255 holds 255.  On the heap, exactly L * 512 bytes: a
// load beyond it is an error under the sanitizer
static std::vector<uint8_t> halving_table(uint32_t L) {
    std::vector<uint8_t> t((size_t)L * kRescaleRow);
    for (uint32_t p = 0; p < L; ++p)
        for (uint32_t q = 0; q < 256; ++q) {
            t[((size_t)p * 256 + q) * 2 + RS_CT] = q == 255 ? 255 : (uint8_t)(q / 2);
            t[((size_t)p * 256 + q) * 2 + RS_GA] = q == 255 ? 255 : (uint8_t)(q < 3 ? 0 : q - 3);
        }
    return t;
}
struct Out { std::vector<uint8_t> quals; RescaleTally t; unsigned long long bins[kRescaleBins] = {}; };
static Out run(const std::vector<uint32_t>& ops, const std::string& read, const std::vector<uint8_t>& quals, const std::vector<uint8_t>& table) {
    HitRec h{};
    h.n_ops = (uint32_t)ops.size(); h.ops_off = 0;
    // exact-size heap copies: a load or a store one byte beyond the read or its qualities is an error under the sanitizer
    std::vector<uint8_t> r(read.begin(), read.end());
    Out o;
    o.quals = quals;
    rescale_read(h, ops.data(), r.data(), quals.data(), o.quals.data(), (uint32_t)r.size(), table.empty() ? nullptr : table.data(), o.t, o.bins);
    return o;
}
static unsigned long long total(const Out& o) { unsigned long long s = 0; for (auto v : o.bins) s += v; return s; }

int main() {
    {   // the two cells and nothing else
        const char B[5] = {'A', 'C', 'G', 'T', 'N'};
        int candidates = 0;
        for (char r : B) for (char q : B) {
            const uint8_t read[1] = {(uint8_t)q};
            uint32_t p = 99;
            const uint32_t c = rescale_column(pack_op(OP_MISMATCH, 0, (uint8_t)r), read, 1, p);
            candidates += c != kRescaleNoCell;
            CHECK((c == RS_CT) == (r == 'C' && q == 'T') && (c == RS_GA) == (r == 'G' && q == 'A') && p == 0);
            CHECK(rescale_column(pack_op(OP_MATCH, 0, 0), read, 1, p) == kRescaleNoCell);  // a match is never a candidate
        }
        CHECK(candidates == 2);
    }
    {   // the column rule on a hand-made track: read 5' CTGANcta 3'
        const std::string read = "CTGANcta";
        const std::vector<uint8_t> quals = {30, 31, 32, 33, 34, 35, 36, 37};
        const auto T = halving_table(8);
        const std::vector<uint32_t> ops = {
            pack_op(OP_MATCH, 0, 0),         // C = C: a match, nothing
            pack_op(OP_MISMATCH, 1, 'C'),    // ref C, read T    -> C->T at 1
            pack_op(OP_INS, 2, 0),           // an insertion of the read's G: nothing
            pack_op(OP_DEL, 2, 'C'),         // a deleted C: nothing
            pack_op(OP_MISMATCH, 3, 'g'),    // ref g (lower case), read A -> G->A at 3, behind an insertion and a deletion
            pack_op(OP_MISMATCH, 4, 'C'),    // read N: nothing
            pack_op(OP_MATCH, 5, 0),         // read c: a match, nothing
            pack_op(OP_MISMATCH, 6, 'c'),    // ref c, read t (both lower case) -> C->T at 6
            pack_op(OP_MISMATCH, 7, 'G'),    // ref G, read a (lower case) -> G->A at 7
            pack_op(OP_MATCH, 8, 0),         // p >= L: nothing, and nothing is read
            pack_op(OP_MISMATCH, 8, 'C'),
            pack_op(OP_MISMATCH, 0xFFFF, 'C'),
            pack_op(OP_MISMATCH, 2, 'A'),    // ref A, read G: not a candidate
            pack_op(OP_MISMATCH, 1, 'G'),    // ref G, read T: not a candidate
        };
        const Out o = run(ops, read, quals, T);
        CHECK(o.t.cols[RS_CT] == 2 && o.t.cols[RS_GA] == 2 && o.t.changed == 4);
        CHECK((o.quals == std::vector<uint8_t>{30, 15, 32, 30, 34, 35, 18, 34}));
        CHECK(o.t.drop == 16 + 3 + 18 + 3);
        CHECK(o.bins[15] == 1 && o.bins[30] == 1 && o.bins[18] == 1 && o.bins[34] == 1 && total(o) == 4);
        // the same track in any order gives the same bytes
        const Out rev = run(std::vector<uint32_t>(ops.rbegin(), ops.rend()), read, quals, T);
        CHECK(rev.quals == o.quals && rev.t.changed == 4 && rev.t.drop == o.t.drop);
        // no table: nothing is a candidate
        const Out none = run(ops, read, quals, {});
        CHECK(none.quals == quals && none.t.cols[0] == 0 && none.t.cols[1] == 0 && none.t.changed == 0 && total(none) == 0);
    }
    {   // the quality byte indexes the row: 0, 1, 93, 94, 254 and 255
        const std::string read = "TTTTTT";
        const auto T = halving_table(6);
        std::vector<uint32_t> ops;
        for (uint32_t p = 0; p < 6; ++p) ops.push_back(pack_op(OP_MISMATCH, p, 'C'));
        const Out o = run(ops, read, {0, 1, 93, 94, 254, 255}, T);
        CHECK((o.quals == std::vector<uint8_t>{0, 0, 46, 47, 127, 255}));
        CHECK(o.t.cols[RS_CT] == 6 && o.t.changed == 4 && o.t.drop == 1 + 47 + 47 + 127);  // q = 0 stays 0, the missing quality stays missing: neither changed
        CHECK(o.bins[0] == 1 && o.bins[46] == 1 && o.bins[47] == 1 && o.bins[63] == 1 && total(o) == 4);  // 127 lands in the last bin
        CHECK(rescale_bin(62) == 62 && rescale_bin(63) == 63 && rescale_bin(64) == 63 && rescale_bin(254) == 63);
        CHECK(rescale_lookup(nullptr, 7, 255, RS_GA) == 255);  // a missing quality loads nothing
    }
    {   // L = 1
        const auto T = halving_table(1);
        CHECK(run({pack_op(OP_MISMATCH, 0, 'C')}, "T", {40}, T).quals[0] == 20);
        CHECK(run({pack_op(OP_MISMATCH, 0, 'G')}, "A", {40}, T).quals[0] == 37);
        CHECK(run({pack_op(OP_MISMATCH, 1, 'C')}, "T", {40}, T).quals[0] == 40);
        CHECK(run({}, "T", {40}, T).quals[0] == 40);
    }
    {   // what reads add to an accumulator
        unsigned long long w[kRescaleWords] = {};
        RescaleTally t;
        t.cols[RS_CT] = 3; t.cols[RS_GA] = 1; t.changed = 2; t.drop = 40;
        rescale_account(true, t, w);
        rescale_account(true, t, w);
        rescale_account(false, t, w);  // a read that is not rescaled: seen, nothing else
        CHECK(w[RS_READS_SEEN] == 3 && w[RS_READS_RESCALED] == 2 && w[RS_COLS_CT] == 6 && w[RS_COLS_GA] == 2 && w[RS_CHANGED] == 4 && w[RS_DROP_SUM] == 80);
    }
    {   // the table rule
        mapad_params_t p;
        std::memset(&p, 0, sizeof p);
        p.model_kind = MAPAD_MODEL_TEST; p.deam_score = -0.5f; p.mm_score = -1.0f; p.match_score = 0.0f;
        // pd = 1 - 2^-0.5 = 0.2929: Q40 -> e' = 0.29296 -> 5.33 + 0.5 -> 5; G->A is scored alike by both models: the identity
        CHECK(std::fabs(host::sdm_prob(p, 0, 3, 'C', 'T', 40, false) - std::exp2(-0.5)) < 1e-15 && host::sdm_prob(p, 0, 3, 'C', 'T', 40, true) == 0.5);
        std::vector<uint8_t> t;
        host::rescale_table(p, 3, t);
        CHECK(t.size() == 3 * kRescaleRow);
        for (int i = 0; i < 3; ++i)
            for (int q = 0; q < 256; ++q) {
                const uint8_t ct = t[((size_t)i * 256 + q) * 2 + RS_CT], ga = t[((size_t)i * 256 + q) * 2 + RS_GA];
                CHECK(ga == q && ct <= q);
                // by hand: Q1 e' = 0.8545 -> 0.68 + 0.5 -> 1; Q2 e' = 0.7390 -> 1.31 + 0.5 -> 1; Q10 e' = 0.3636 -> 4.39 + 0.5 -> 4; from Q11 on 5.07 ... 5.83 -> 5
                if (q == 0) CHECK(ct == 0);
                if (q == 1 || q == 2) CHECK(ct == 1);
                if (q == 10) CHECK(ct == 4);
                if (q == 11 || q == 40 || q == 93 || q == 94 || q == 254) CHECK(ct == 5);
                if (q == 255) CHECK(ct == 255);
            }
        // e' >= 1: a null model that gives the column no probability at all (pd = 1) -> 0 for every quality; q = 0 (e = 1) -> 0 under any posterior
        p.deam_score = 0.0f; p.mm_score = -INFINITY;
        CHECK(host::rescale_quality(p, 0, 1, 0, 40) == 0 && host::rescale_quality(p, 0, 1, 0, 254) == 0 && host::rescale_quality(p, 0, 1, 0, 1) == 0);
        p.deam_score = -0.5f; p.mm_score = -1.0f;
        CHECK(host::rescale_quality(p, 0, 1, 0, 0) == 0);
        // P_dam <= P_null: the identity
        p.deam_score = -2.0f;
        for (int q = 0; q < 255; ++q) CHECK(host::rescale_quality(p, 0, 1, 0, q) == q);
        // the quality-aware model: never above q, the identity without damage, 255 kept, and Q254 (e = 10^-25.4, below an ulp of 1) stays exact without damage
        std::memset(&p, 0, sizeof p);
        p.model_kind = MAPAD_MODEL_SIMPLE_ADNA; p.library_prep = MAPAD_LIBRARY_SINGLE_STRANDED; p.five_prime_overhang = 0.5f; p.three_prime_overhang = 0.5f;
        p.ds_deamination_rate = 0.02f; p.ss_deamination_rate = 1.0f; p.divergence = 0.02f / 3.0f;
        t.clear();
        host::rescale_table(p, 20, t);
        bool changed = false;
        for (int i = 0; i < 20; ++i)
            for (int q = 0; q < 256; ++q)
                for (int c = 0; c < 2; ++c) {
                    const uint8_t v = t[((size_t)i * 256 + q) * 2 + c];
                    CHECK(v <= q && (q != 255 || v == 255));
                    changed = changed || v != q;
                }
        CHECK(changed && t[(0 * 256 + 37) * 2 + RS_CT] < t[(10 * 256 + 37) * 2 + RS_CT]);  // the 5' end is marked down further than the middle
        for (int i = 1; i < 20; ++i) for (int q = 0; q < 256; ++q) CHECK(t[((size_t)i * 256 + q) * 2 + RS_GA] == t[(size_t)q * 2 + RS_GA]);  // G->A: the -d rate at every position
        p.ds_deamination_rate = 0.0f; p.ss_deamination_rate = 0.0f;
        t.clear();
        host::rescale_table(p, 20, t);
        for (int i = 0; i < 20; ++i) for (int q = 0; q < 256; ++q) for (int c = 0; c < 2; ++c) CHECK(t[((size_t)i * 256 + q) * 2 + c] == q);
    }
    std::printf("rescale selftest ok\n");
    return 0;
}
