// clean_selftest.cpp — clean_core.hpp driven the way clean_decide_kernel drives it, against a base-by-base serial restatement of the rule.
// 64 emulated lanes: every trip's ballots are built from the lanes' predicates, shuffles read the neighbouring lanes' values, and each lane calls the core's lane
// functions (poly_x, poly_stop, poly_candidate, poly_trip_tail, run_length, dust_counted, dust_code, dust_lane_pairs, dust_score) exactly as the kernel does.
// Checked against the restatement below and against clean::decide (the host path's one-thread driver): class, trim5, trim3, poly_len, dust and the output range,
// over the shapes of the tests' table and 20 000 random reads of 0 .. 1100 bases with planted tails and repeats.
// Stand-alone (own main), built with -fsanitize=address,undefined by tests/test_clean_host.py: every index the emulated kernel forms is checked on the way.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../mapad_amd/csrc/clean_core.hpp"

using namespace mapad;
typedef std::vector<uint8_t> Bytes;

static bool valid(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// ---- the serial restatement -------------------------------------------------------------------------------------------------------------------------------
struct Out { uint32_t cls, trim5, trim3, poly, dust, src, len; };
static uint32_t serial_window(const uint8_t* w, uint32_t len) {
    std::map<std::string, uint32_t> count;
    for (uint32_t i = 0; i + 2 < len; ++i)
        if (valid(w[i]) && valid(w[i + 1]) && valid(w[i + 2])) count[std::string((const char*)w + i, 3)] += 1;
    uint32_t T = 0, S = 0;
    for (auto& kv : count) { T += kv.second; S += kv.second * (kv.second - 1) / 2; }
    return T < 2 ? 0 : 2000 * S / (T * (T - 1));
}
static Out serial(const clean::Rule& R, const Bytes& r, const Bytes& q) {
    Out o{};
    const uint32_t L = (uint32_t)r.size();
    if (L == 0) { o.cls = clean::CLS_EMPTY; return o; }
    if (L > 1024) { o.cls = clean::CLS_TOO_LONG; o.len = L; return o; }
    if (R.ops & clean::OP_POLY) {
        uint32_t x = 0;
        for (uint32_t n = 1; n <= L; ++n) {
            x += r[L - n] != R.poly_base;
            if (x > R.poly_max_mismatch || (n >= R.poly_min_len && (uint64_t)x * R.poly_one_in > n)) break;
            if (n >= R.poly_min_len && r[L - n] == R.poly_base) o.poly = n;
        }
    }
    auto rem = [&](uint32_t i) {
        return ((R.ops & clean::OP_TRIM_N) && !valid(r[i])) || ((R.ops & clean::OP_TRIM_QUAL) && q[i] != 255 && q[i] <= R.min_quality);
    };
    uint32_t lo = 0, hi = L - o.poly;
    while (hi > lo && rem(hi - 1)) --hi;
    while (lo < hi && rem(lo)) ++lo;
    o.trim5 = lo; o.trim3 = L - hi;
    const uint32_t M = hi - lo;
    if (M < R.min_length) { o.cls = clean::CLS_TOO_SHORT; return o; }
    if (R.ops & clean::OP_DUST)
        for (uint32_t k = 0;; ++k) {
            const uint32_t b = 32 * k, e = std::min(b + 64, M);
            if (b < e) o.dust = std::max(o.dust, serial_window(r.data() + lo + b, e - b));
            if (32 * k + 64 >= M) break;
        }
    if ((R.ops & clean::OP_DUST) && o.dust > R.max_dust) { o.cls = clean::CLS_LOW_COMPLEXITY; return o; }
    o.cls = M < L ? clean::CLS_TRIMMED : clean::CLS_KEPT; o.src = lo; o.len = M;
    return o;
}

// ---- the kernel's way --------------------------------------------------------------------------------------------------------------------------------------
static uint64_t ballot(const bool pred[64]) { uint64_t m = 0; for (int l = 0; l < 64; ++l) if (pred[l]) m |= 1ull << l; return m; }
static Out wave(const clean::Rule& R, const Bytes& rb, const Bytes& qb) {
    Out o{};
    const uint64_t len = rb.size();
    if (len == 0) { o.cls = clean::CLS_EMPTY; return o; }
    if (len > (uint64_t)clean::kMaxLen) { o.cls = clean::CLS_TOO_LONG; o.len = (uint32_t)len; return o; }
    const uint32_t L = (uint32_t)len;
    const uint8_t* s = rb.data();  // exactly-sized: an index past the read is the sanitizer's to find
    const uint8_t* q = qb.data();
    uint32_t poly = 0, t3 = 0, t5 = 0, dust = 0;
    if (R.ops & clean::OP_POLY) {
        uint32_t carry = 0;
        for (uint32_t t = 0; 64u * t < L; ++t) {
            bool p_not[64], p_stop[64], p_cand[64];
            uint8_t b[64];
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t n = 64u * t + lane + 1u;
                const bool in = n <= L;
                b[lane] = in ? s[L - n] : (uint8_t)0;
                p_not[lane] = in && b[lane] != (uint8_t)R.poly_base;
            }
            const uint64_t not_base = ballot(p_not);
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t n = 64u * t + lane + 1u;
                const bool in = n <= L;
                const uint32_t x = clean::poly_x(not_base, carry, lane);
                p_stop[lane] = !in || clean::poly_stop(R, n, x);
                p_cand[lane] = in && clean::poly_candidate(R, n, b[lane]);
            }
            const uint64_t stop = ballot(p_stop), cand = ballot(p_cand);
            const uint32_t tail = clean::poly_trip_tail(stop, cand, t);
            if (tail) poly = tail;
            if (stop) break;
            carry += (uint32_t)clean::popc64(not_base);
        }
    }
    const uint32_t E = L - poly;
    if (R.ops & (clean::OP_TRIM_N | clean::OP_TRIM_QUAL)) {
        for (uint32_t base = 0; base < E; base += 64u) {
            bool p[64];
            for (uint32_t lane = 0; lane < 64; ++lane) { const uint32_t i = base + lane; p[lane] = i < E && clean::removable(R, s[E - 1u - i], q[E - 1u - i]); }
            const uint32_t run = clean::run_length(ballot(p));
            t3 += run;
            if (run < 64u) break;
        }
        const uint32_t E5 = E - t3;
        for (uint32_t base = 0; base < E5; base += 64u) {
            bool p[64];
            for (uint32_t lane = 0; lane < 64; ++lane) { const uint32_t i = base + lane; p[lane] = i < E5 && clean::removable(R, s[i], q[i]); }
            const uint32_t run = clean::run_length(ballot(p));
            t5 += run;
            if (run < 64u) break;
        }
    }
    const uint32_t M = E - t3 - t5;
    if (M >= R.min_length && (R.ops & clean::OP_DUST)) {
        const uint8_t* w = s + t5;
        for (uint32_t k = 0;; ++k) {
            uint32_t c0[64], code[64];
            bool counted[64], bit[6][64];
            for (uint32_t lane = 0; lane < 64; ++lane) { const uint32_t i = 32u * k + lane; c0[lane] = i < M ? (uint32_t)base_index(w[i]) : 4u; }
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t c1 = c0[lane + 1 < 64 ? lane + 1 : lane], c2 = c0[lane + 2 < 64 ? lane + 2 : lane];  // a shuffle from past the wavefront gives the lane's own value
                counted[lane] = clean::dust_counted(lane, c0[lane], c1, c2);
                code[lane] = counted[lane] ? clean::dust_code(c0[lane], c1, c2) : 0u;
                for (int b = 0; b < 6; ++b) bit[b][lane] = counted[lane] && ((code[lane] >> b) & 1u);
            }
            const uint64_t C = ballot(counted);
            uint64_t B[6];
            for (int b = 0; b < 6; ++b) B[b] = ballot(bit[b]);
            uint32_t S = 0;
            for (uint32_t lane = 0; lane < 64; ++lane) S += counted[lane] ? clean::dust_lane_pairs(B, C, code[lane], lane) : 0u;
            const uint32_t score = clean::dust_score(S, (uint32_t)clean::popc64(C));
            dust = std::max(dust, score);
            if (clean::dust_last_window(k, M)) break;
        }
    }
    o.poly = poly; o.trim5 = t5; o.trim3 = t3 + poly; o.dust = dust;
    o.cls = clean::final_class(R, L, M, dust);
    if (clean::yields_read(o.cls)) { o.len = M; o.src = t5; }
    return o;
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static int n_reads = 0;
static uint64_t class_seen[clean::N_CLASSES] = {0};
static void check_read(const clean::Rule& R, const Bytes& r, const Bytes& q, const char* what) {
    const Out a = serial(R, r, q), b = wave(R, r, q);
    const clean::Decision D = clean::decide(R, r.data(), q.data(), r.size());
    ++n_reads;
    class_seen[a.cls] += 1;
    CHECK(a.cls == b.cls && a.trim5 == b.trim5 && a.trim3 == b.trim3 && a.poly == b.poly && a.dust == b.dust && a.len == b.len && a.src == b.src,
          "%s: L %zu ops %u: lanes cls %u t5 %u t3 %u poly %u dust %u len %u, serial cls %u t5 %u t3 %u poly %u dust %u len %u", what, r.size(), R.ops, b.cls, b.trim5, b.trim3,
          b.poly, b.dust, b.len, a.cls, a.trim5, a.trim3, a.poly, a.dust, a.len);
    CHECK(a.cls == D.cls && a.trim5 == D.trim5 && a.trim3 == D.trim3 && a.poly == D.poly_len && a.dust == D.dust && a.len == D.out_len && a.src == D.src,
          "%s: L %zu ops %u: decide() cls %u t5 %u t3 %u poly %u dust %u len %u, serial cls %u t5 %u t3 %u poly %u dust %u len %u", what, r.size(), R.ops, D.cls, D.trim5,
          D.trim3, D.poly_len, D.dust, D.out_len, a.cls, a.trim5, a.trim3, a.poly, a.dust, a.len);
}

int main() {
    std::mt19937_64 rng(2024);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    auto bases = [&](int n, int dirty_permille) {
        Bytes s((size_t)n);
        for (auto& c : s) { c = (uint8_t)"ACGT"[rng() & 3]; if (rnd(0, 999) < dirty_permille) c = (uint8_t)"NRYacgt."[rng() & 7]; }
        return s;
    };
    auto quals = [&](int n, int low_percent) {
        Bytes q((size_t)n);
        for (auto& c : q) { const int k = rnd(0, 99); c = k < low_percent ? (uint8_t)rnd(0, 3) : k == 99 ? 255 : (uint8_t)rnd(4, 41); }
        return q;
    };
    auto fill = [&](Bytes& s, int from, int to, const std::string& unit) { for (int i = from; i < to; ++i) s[(size_t)i] = (uint8_t)unit[(size_t)(i - from) % unit.size()]; };
    const clean::Rule defaults{clean::OP_ALL, 'G', 10, 8, 5, 2, 15, 70};
    std::vector<clean::Rule> rules;
    for (uint32_t ops : {1u, 2u, 4u, 8u, 0u, 6u, 15u}) { clean::Rule R = defaults; R.ops = ops; rules.push_back(R); }
    rules.push_back(clean::Rule{clean::OP_ALL, 'A', 1, 1, 0, 0, 0, 0});
    rules.push_back(clean::Rule{clean::OP_ALL, 'G', 20, 4, 40, 20, 3, 1000});
    rules.push_back(clean::Rule{clean::OP_ALL, 'T', 64, 0xFFFFFFFFu, 0xFFFFFFFFu, 93, 1, 320});

    // the shapes of the table: the lengths around the trips and the windows, as random bases, as one tail, as one homopolymer, as N; tails at every length around a trip
    for (const clean::Rule& R : rules) {
        for (int L : {0, 1, 2, 3, 14, 15, 63, 64, 65, 95, 96, 97, 127, 128, 129, 1023, 1024, 1025}) {
            check_read(R, bases(L, 0), quals(L, 0), "random");
            check_read(R, Bytes((size_t)L, 'G'), quals(L, 0), "all G");
            check_read(R, Bytes((size_t)L, 'A'), quals(L, 0), "all A");
            check_read(R, Bytes((size_t)L, 'N'), quals(L, 0), "all N");
            check_read(R, bases(L, 0), Bytes((size_t)L, 2), "all low");
            for (const char* unit : {"AC", "ACG", "ACGT"}) { Bytes s((size_t)L); fill(s, 0, L, unit); check_read(R, s, quals(L, 0), "repeat"); }
        }
        for (int tail = 1; tail <= 200; ++tail)
            for (int body : {0, 1, 30}) {
                Bytes s = bases(body + tail, 0);
                if (body) s[(size_t)body - 1] = 'A';
                fill(s, body, body + tail, "G");
                check_read(R, s, quals(body + tail, 0), "tail");
                // one other base at every 8th place of the tail, and the same one place early
                Bytes m = s, e = s;
                for (int k = 8; k <= tail; k += 8) { m[(size_t)(body + tail - k)] = 'C'; e[(size_t)(body + tail - k + 1)] = 'C'; }
                check_read(R, m, quals(body + tail, 0), "tail, one in eight");
                check_read(R, e, quals(body + tail, 0), "tail, one early");
            }
        // ends of 0 .. 130 removable bases on either side of 40 good ones
        for (int a = 0; a <= 130; a += (a < 4 || (a > 60 && a < 68) || a > 125) ? 1 : 7)
            for (int b : {0, 1, 63, 64, 65, 130}) {
                Bytes s = bases(a + 40 + b, 0), q((size_t)(a + 40 + b), 30);
                for (int i = 0; i < a; ++i) { if (i & 1) s[(size_t)i] = 'N'; else q[(size_t)i] = 1; }
                for (int i = 0; i < b; ++i) { if (i & 1) q[(size_t)(a + 40 + i)] = 0; else s[(size_t)(a + 40 + i)] = 'N'; }
                check_read(R, s, q, "ends");
            }
        // a repeat in one stretch of 97 bases, every start
        for (int at = 0; at <= 80; ++at) { Bytes s = bases(97, 0); fill(s, at, std::min(97, at + 33), at & 1 ? "A" : "CA"); check_read(R, s, quals(97, 0), "window"); }
    }
    // random reads of 0 .. 1100 bases with planted tails, repeats, bad ends, under the default rule and under random ones
    for (int it = 0; it < 20000; ++it) {
        clean::Rule R = rules[(size_t)it % rules.size()];
        if (it % 3 == 0) R = clean::Rule{(uint32_t)rnd(0, 15), (uint32_t)"ACGT"[rng() & 3], (uint32_t)rnd(1, 70), (uint32_t)rnd(1, 12), (uint32_t)rnd(0, 8), (uint32_t)rnd(0, 93),
                                         (uint32_t)rnd(0, 40), (uint32_t)rnd(0, 1000)};
        const int L = it % 10 == 0 ? rnd(0, 1100) : rnd(0, 200);
        Bytes s = bases(L, it % 4 == 0 ? 30 : 0), q = quals(L, it % 5 == 0 ? 30 : 2);
        if (L && it % 2 == 0) {  // a tail of the rule's base with a few other bases in it
            const int t = rnd(1, L);
            for (int i = L - t; i < L; ++i) if (rnd(0, 15)) s[(size_t)i] = (uint8_t)R.poly_base;
        }
        if (L && it % 3 == 1) { const int a = rnd(0, L - 1), b = rnd(a, L); fill(s, a, b, std::string("ACGTTGA").substr((size_t)rnd(0, 3), (size_t)rnd(1, 4))); }
        if (L && it % 7 == 0) { const int a = rnd(0, std::min(L, 70)); for (int i = 0; i < a; ++i) s[(size_t)i] = 'N'; }
        if (L && it % 11 == 0) { const int b = rnd(0, std::min(L, 70)); for (int i = L - b; i < L; ++i) q[(size_t)i] = (uint8_t)rnd(0, 2); }
        check_read(R, s, q, "random");
    }
    for (uint32_t k = 0; k < clean::N_CLASSES; ++k) CHECK(class_seen[k] > 100, "class %u occurred %llu times", k, (unsigned long long)class_seen[k]);
    if (failures) { std::printf("clean selftest: %d failures over %d reads\n", failures, n_reads); return 1; }
    std::printf("clean selftest ok: %d reads\n", n_reads);
    return 0;
}
