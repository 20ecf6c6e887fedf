// text_selftest.cpp — the formatting code of the text kernel (mapad_amd/csrc/text_core.hpp: TextSink, bam_fields_hd, xa_entry_hd) driven directly on the host:
// the numbers against snprintf, CIGAR / MD / NM of hand-written edit tracks against strings worked out by hand and against the host restatement
// (host_postproc.hpp: to_bam_fields, which looks original symbols up in a map where the kernel merges two sorted arrays).  A stand-alone program
// (tests/test_records_host.py builds it with -fsanitize=address,undefined and runs it as a child process); exits 0 and prints "text selftest ok" when every
// check holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../mapad_amd/csrc/host_postproc.hpp"

using namespace mapad;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// ---- numbers ---------------------------------------------------------------------------------------------------------------------------------------------
template <class F>
static std::string sunk(F put) {  // count first, then write into a heap buffer of exactly that size: a byte too many is an error under the sanitizer
    TextSink count{nullptr, 0, false};
    put(count);
    std::vector<char> buf(count.n);
    TextSink w{buf.data(), 0, true};
    put(w);
    CHECK(w.n == count.n);
    return std::string(buf.begin(), buf.end());
}
static void check_f2(float x) {
    char want[400];
    std::snprintf(want, sizeof want, "%.2f", (double)x);
    const std::string got = sunk([&](TextSink& s) { s.put_f2(x); });
    if (got != want) { std::fprintf(stderr, "put_f2(%a): \"%s\", snprintf \"%s\"\n", (double)x, got.c_str(), want); std::exit(1); }
}
static void check_u64(uint64_t v) {
    char want[32];
    std::snprintf(want, sizeof want, "%llu", (unsigned long long)v);
    const std::string got = sunk([&](TextSink& s) { s.put_u64(v); });
    if (got != want) { std::fprintf(stderr, "put_u64: \"%s\", snprintf \"%s\"\n", got.c_str(), want); std::exit(1); }
}
static void numbers() {
    check_f2(0.0f); check_f2(-0.0f);
    for (float t : {-1e-30f, -1e-10f, -0.001f, -0.004999f, -0.005f, -0.0050001f, 1e-30f, 0.004999f, 0.005f, 0.0050001f, -1.17549435e-38f, -1e-45f}) check_f2(t);  // "-0.00" keeps its sign
    for (int k = -80000; k <= 80000; ++k) check_f2((float)k / 8.0f);      // x.125, x.375, x.625, x.875 are exact: ties, to even
    for (int k = -4000; k <= 4000; ++k) check_f2((float)k / 16.0f + (k < 0 ? -256.0f : 256.0f));
    for (int k = -3200; k <= 3200; ++k) check_f2((float)k / 200.0f);      // x.xx5 as a float: never a tie, the nearest float decides
    for (float p = 1.0f; p <= 1e9f; p *= 10.0f)                           // near the powers of ten: 9.99|5, 99.99|5, ...
        for (float c : {p - 0.01f, p - 0.005f, p - 0.004f, p - 0.006f, p, p + 0.004f, p + 0.005f})
            for (float s : {1.0f, -1.0f}) {
                check_f2(s * c); check_f2(s * std::nextafterf(c, 0.0f)); check_f2(s * std::nextafterf(c, 2.0f * c));
            }
    check_f2(-16777216.0f); check_f2(-3.4e12f); check_f2(1.8e16f);
    std::mt19937_64 rng(7);
    for (int i = 0; i < 1000000; ++i) {  // negative scores: uniform over [-64, 0), and uniform over the bit patterns of [2^-20, 2^7)
        const uint64_t r = rng();
        check_f2(-(float)((double)(r >> 11) * (64.0 / 9007199254740992.0)));
        uint32_t bits = 0x80000000u | ((107u + (uint32_t)((r >> 32) % 27u)) << 23) | ((uint32_t)r & 0x7FFFFFu);
        float f;
        std::memcpy(&f, &bits, 4);
        check_f2(f);
    }
    check_u64(0);
    uint64_t p = 1;
    for (int d = 1; d <= 19; ++d) { p *= 10; check_u64(p - 1); check_u64(p); check_u64(p + 1); }  // 9 | 10 ... 10^19 - 1 | 10^19
    check_u64(0xFFFFFFFFull); check_u64(0x100000000ull); check_u64(0x7FFFFFFFFFFFFFFFull); check_u64(0xFFFFFFFFFFFFFFFFull);
    for (int i = 0; i < 100000; ++i) check_u64(rng() >> (rng() % 64));
}

// ---- CIGAR / MD / NM ---------------------------------------------------------------------------------------------------------------------------------------
struct Symbols {  // original symbols, both ways: the kernel's sorted arrays (exact-size heap copies) and the host index's map
    std::vector<uint64_t> pos;
    std::vector<uint8_t> sym;
    host::Index ix;
    void add(uint64_t p, char c) { CHECK(pos.empty() || pos.back() < p); pos.push_back(p); sym.push_back((uint8_t)c); ix.original_symbols[p] = (uint8_t)c; }
    TextIndex view() const { return TextIndex{pos.data(), sym.data(), pos.size(), nullptr, nullptr}; }
};
struct Fields { std::string cigar, md; int32_t nm; };
static Fields device_fields(const Symbols& S, const std::vector<uint32_t>& ops, bool backward, uint64_t abs) {
    const TextIndex T = S.view();
    const uint32_t n = (uint32_t)ops.size();
    TextSink c0{nullptr, 0, false}, m0{nullptr, 0, false};
    const int32_t nm = bam_fields_hd(T, ops.data(), n, backward, abs, &c0, &m0);
    std::vector<char> cb(c0.n), mb(m0.n);
    TextSink c1{cb.data(), 0, true}, m1{mb.data(), 0, true};
    CHECK(bam_fields_hd(T, ops.data(), n, backward, abs, &c1, &m1) == nm && c1.n == c0.n && m1.n == m0.n);
    // one at a time, as an XA entry asks for them
    std::vector<char> cb2(c0.n), mb2(m0.n);
    TextSink c2{cb2.data(), 0, true}, m2{mb2.data(), 0, true};
    bam_fields_hd(T, ops.data(), n, backward, abs, &c2, nullptr);
    CHECK(bam_fields_hd(T, ops.data(), n, backward, abs, nullptr, &m2) == nm && cb2 == cb && mb2 == mb);
    return Fields{std::string(cb.begin(), cb.end()), std::string(mb.begin(), mb.end()), nm};
}
static Fields both(const Symbols& S, const std::vector<uint32_t>& ops, bool backward, uint64_t abs) {
    const Fields d = device_fields(S, ops, backward, abs);
    const host::BamFields h = host::to_bam_fields(host::Track{ops.data(), (uint32_t)ops.size()}, backward, abs, S.ix);
    if (d.cigar != h.cigar || d.md != h.md || d.nm != h.nm) {
        std::fprintf(stderr, "device %s %s %d, host %s %s %d\n", d.cigar.c_str(), d.md.c_str(), d.nm, h.cigar.c_str(), h.md.c_str(), h.nm);
        std::exit(1);
    }
    return d;
}
static void expect(const Fields& f, const char* cigar, const char* md, int32_t nm) {
    if (f.cigar != cigar || f.md != md || f.nm != nm) { std::fprintf(stderr, "got %s %s %d, expected %s %s %d\n", f.cigar.c_str(), f.md.c_str(), f.nm, cigar, md, nm); std::exit(1); }
}
static uint32_t M(uint32_t j) { return pack_op(OP_MATCH, j, 0); }
static uint32_t X(uint32_t j, char ref) { return pack_op(OP_MISMATCH, j, (uint32_t)ref); }
static uint32_t I(uint32_t j) { return pack_op(OP_INS, j, 0); }
static uint32_t D(uint32_t j, char ref) { return pack_op(OP_DEL, j, (uint32_t)ref); }

static void tracks() {
    {   // no symbols at all
        Symbols S;
        expect(both(S, {M(0), X(1, 'G'), M(2)}, false, 7), "3M", "1G1", 1);
        expect(both(S, {M(0), X(1, 'G'), M(2), M(3)}, true, 7), "4M", "2C1", 1);  // the other strand: from the track's end, complemented
        expect(both(S, {X(0, 'a')}, true, 0), "1M", "0t0", 1);
        expect(both(S, {}, false, 0), "", "0", 0);
    }
    {   // an insertion in front of an original symbol: operations are counted, insertions included, when the symbol is looked up (record.rs:301-320) — the
        // fourth operation meets the symbol of text position abs + 3 although it aligns to abs + 2, whose own symbol nothing looks at
        Symbols S;
        S.add(990, 'W'); S.add(999, 'K'); S.add(1002, 'Y'); S.add(1003, 'R'); S.add(1005, 'S');  // in front of the alignment, under the insertion, the one that counts, behind the track
        const std::vector<uint32_t> ops = {M(0), M(1), I(2), M(3), M(4)};
        expect(both(S, ops, false, 1000), "2M1I2M", "2R1", 2);
        expect(both(S, ops, true, 1000), "2M1I2M", "2Y1", 2);  // the track read from its end is M M I M M again; the other strand shows R's complement
    }
    {   // a deletion run across a symbol: the deleted base is shown as the symbol, the run goes on
        Symbols S;
        S.add(503, 'N');
        const std::vector<uint32_t> ops = {M(0), M(1), D(2, 'A'), D(2, 'C'), D(2, 'G'), M(2), M(3)};
        expect(both(S, ops, false, 500), "2M3D2M", "2^ANG2", 3);
        expect(both(S, ops, true, 500), "2M3D2M", "2^CNT2", 3);  // from the end: G C A complemented, the second of them on the symbol
        S.add(504, 'B');
        expect(both(S, ops, false, 500), "2M3D2M", "2^ANB2", 3);
        S.add(505, 'H');  // the match behind the run becomes a mismatch: "0" between a deletion and a mismatch
        expect(both(S, ops, false, 500), "2M3D2M", "2^ANB0H1", 4);
    }
    {   // 19 consecutive symbols: a run of N that was replaced base by base
        Symbols S;
        for (uint64_t p = 105; p < 124; ++p) S.add(p, 'N');
        std::vector<uint32_t> ops;
        for (uint32_t j = 0; j < 30; ++j) ops.push_back(M(j));
        std::string md = "5N";
        for (int k = 0; k < 18; ++k) md += "0N";
        md += "6";
        expect(both(S, ops, false, 100), "30M", md.c_str(), 19);
        expect(both(S, ops, true, 100), "30M", md.c_str(), 19);
        ops[10] = X(10, 'C');  // a mismatch on a symbol shows the symbol
        expect(both(S, ops, false, 100), "30M", md.c_str(), 19);
    }
    {   // the other strand with every code
        Symbols S;
        const char* codes = "NRYKMSWBDHVU";
        for (int k = 0; k < 12; ++k) S.add(41 + (uint64_t)k, codes[k]);
        std::vector<uint32_t> ops;
        for (uint32_t j = 0; j < 14; ++j) ops.push_back(M(j));
        expect(both(S, ops, false, 40), "14M", "1N0R0Y0K0M0S0W0B0D0H0V0U1", 12);
        expect(both(S, ops, true, 40), "14M", "1N0Y0R0M0K0S0W0V0H0D0B0U1", 12);
    }
    {   // 32 767 operations, symbols every 37 positions, on both strands
        std::mt19937 rng(11);
        Symbols S;
        for (uint64_t p = 70000; p < 70000 + 40000; p += 37) S.add(p, "NRYKMSWBDHVU"[(p / 37) % 12]);
        std::vector<uint32_t> ops;
        uint32_t j = 0;
        while (ops.size() < 32767) {
            const uint32_t r = rng() % 100, run = 1 + rng() % 6;
            for (uint32_t k = 0; k < run && ops.size() < 32767; ++k) {
                if (r < 80) ops.push_back(M(j++));
                else if (r < 90) ops.push_back(X(j++, "ACGT"[rng() % 4]));
                else if (r < 95) ops.push_back(I(j++));
                else ops.push_back(D(j, "ACGT"[rng() % 4]));
            }
        }
        CHECK(ops.size() == 32767);
        const Fields f = both(S, ops, false, 70011), b = both(S, ops, true, 70011);
        CHECK(f.md.find("^") != std::string::npos && f.cigar.find("I") != std::string::npos && f.nm > 5000 && b.nm > 5000);
        CHECK(f.md.find_first_of("NRYKMSWBDHVU") != std::string::npos && f.cigar != b.cigar);
        std::vector<uint32_t> all_match;
        for (uint32_t q = 0; q < 32767; ++q) all_match.push_back(M(q));
        Symbols none;
        expect(both(none, all_match, false, 5), "32767M", "32767", 0);
    }
    {   // random short tracks against the host restatement: symbols dense and sparse, at the alignment's first and last position and on both sides of it
        std::mt19937 rng(13);
        for (int t = 0; t < 20000; ++t) {
            Symbols S;
            const uint64_t abs = 50 + rng() % 50;
            const uint32_t n = rng() % 80, step = 1 + rng() % 9;
            for (uint64_t p = rng() % 60; p < abs + n + 20; p += 1 + rng() % step) S.add(p, "NRYKMSWBDHVUnrykmswbdhvu"[rng() % 24]);
            std::vector<uint32_t> ops;
            for (uint32_t q = 0; q < n; ++q) {
                const uint32_t r = rng() % 10;
                ops.push_back(r < 5 ? M(q) : r < 7 ? X(q, "ACGTacgt"[rng() % 8]) : r < 8 ? I(q) : D(q, "ACGTacgt"[rng() % 8]));
            }
            both(S, ops, (t & 1) != 0, abs);
        }
    }
}

// ---- one XA entry: name,±pos,CIGAR,MD,NM,size,score; -----------------------------------------------------------------------------------------------------------
static void xa_entry() {
    Symbols S;
    S.add(1003, 'R');
    const std::vector<uint32_t> pool = {M(0), M(1), M(2), M(0), M(1), I(2), M(3), M(4)};  // the hit's track starts at 3
    const std::string names = "firstchrZ";
    const std::vector<uint32_t> name_off = {0, 5, 9};
    TextIndex T = S.view();
    T.name_off = name_off.data(); T.names = names.data();
    HitRec h{};
    h.size = 1234567; h.score = -1.125f; h.n_ops = 5; h.ops_off = 3;
    const CoordOut c{0, 1, 41, 1000, 0, 0};
    CHECK(sunk([&](TextSink& s) { xa_entry_hd(T, c, h, pool.data(), s); }) == "chrZ,+42,2M1I2M,2R1,2,1234567,-1.12;");
    const CoordOut r{0, 0, 0, 1000, 1, 0};
    h.score = -0.375f;
    CHECK(sunk([&](TextSink& s) { xa_entry_hd(T, r, h, pool.data(), s); }) == "first,-1,2M1I2M,2Y1,2,1234567,-0.38;");
}

int main() {
    numbers();
    tracks();
    xa_entry();
    std::printf("text selftest ok\n");
    return 0;
}
