// align_selftest.cpp — the alignment -> track rule of mapad_amd/csrc/align_core.hpp driven directly on the host: tracks written out by hand on either strand, the
// MD tokens at their edges (a zero-length number, lower case, a letter behind a ^ run, numbers too long), more than 64 CIGAR operations, a deletion across
// column 64, one read per status class with the faults of later classes too, and align_md_advance — what a lane of align_build_kernel calls for its own byte —
// against the serial reader.  A stand-alone program (tests/test_analyse_host.py builds it with -fsanitize=address,undefined and runs it as a child process);
// exits 0 and prints "align selftest ok" when every check holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../mapad_amd/csrc/align_core.hpp"

using namespace mapad;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static const uint64_t kStart[2] = {0, 3000}, kEnd[2] = {2999, 4999};  // two contigs of 3000 and 2000 bases, ends inclusive

static std::vector<uint32_t> cigar_words(const std::string& s) {
    std::vector<uint32_t> w;
    uint32_t n = 0;
    for (char c : s) {
        if (c >= '0' && c <= '9') { n = n * 10 + (uint32_t)(c - '0'); continue; }
        const char* at = std::strchr("MIDNSHP=X", c);
        CHECK(at != nullptr);
        w.push_back(n << 4 | (uint32_t)(at - "MIDNSHP=X"));
        n = 0;
    }
    return w;
}
static uint32_t op(uint32_t kind, uint32_t pos, char base = 0) { return kind << 24 | (uint32_t)(uint8_t)base << 16 | pos; }

struct Out {
    uint32_t cls;
    HitRec h;
    CoordRec cr;
    std::vector<uint32_t> ops;  // the read's room (what align_count said), filled with a canary
};
static const uint32_t kCanary = 0xDEADBEEFu;
// one read through align_read, every input an exact-size heap copy: the sanitizer sees a read or a write beyond them
static Out run(const std::string& cigar, const std::string& md, uint32_t L, bool reverse, bool start_at_end = true, int32_t tid = 0, int64_t pos0 = 100, uint16_t flags = 0,
               uint8_t mapq = 37, uint32_t min_mapq = 0, uint64_t x0 = 1) {
    const std::vector<uint32_t> cw = cigar_words(cigar);
    const std::vector<uint8_t> mb(md.begin(), md.end());
    AlignIn a{};
    a.pos0 = pos0; a.x0 = x0; a.cigar_off = 0; a.md_off = 0; a.tid = tid; a.n_cigar = (uint32_t)cw.size(); a.md_len = (uint32_t)mb.size(); a.as_score = -2.5f;
    a.flags = (uint16_t)(flags | (reverse ? 0x10 : 0)); a.mapq = mapq;
    uint32_t n_ops = 0;
    uint64_t ref_len = 0;
    (void)align_count(a, cw.data(), L, 2, min_mapq, n_ops, ref_len);
    Out o;
    o.ops.assign(n_ops, kCanary);
    o.cls = align_read(a, cw.data(), mb.data(), L, kStart, kEnd, 2, min_mapq, start_at_end, 0, o.ops.data(), o.h, o.cr);
    if (o.cls != ALN_OK) {  // seen, not counted: nothing written, nothing mapped
        for (uint32_t w : o.ops) CHECK(w == kCanary);
        CHECK(o.h.n_ops == 0 && o.cr.mapped == 0 && o.cr.first.tid == -1 && o.cr.x0 == 0 && o.cr.error == 0);
    } else {
        CHECK(o.h.n_ops == n_ops && o.h.size == (x0 ? x0 : 1) && o.h.score == -2.5f && o.h.lower == 0 && o.h.lower_rev == 0 && o.h.ops_off == 0);
        CHECK(o.cr.mapped == 1 && o.cr.best == 0 && o.cr.first.tid == tid && o.cr.first.rel == (uint64_t)pos0 && o.cr.first.abs == kStart[tid] + (uint64_t)pos0);
        CHECK(o.cr.first.backward == (reverse ? 1u : 0u) && o.cr.x0 == (x0 ? x0 : 1) && o.cr.x1 == 0 && o.cr.n_xa == 0 && o.cr.n_order == 0 && o.cr.error == 0);
        for (uint32_t w : o.ops) CHECK(w != kCanary);
        // the walks the stages do: reference order is track order, reversed for a reverse record; the columns are the CIGAR's span
        uint64_t span = 0;
        for (uint32_t i = 0; i < n_ops; ++i) span += (coverage_ref_op(o.ops.data(), n_ops, reverse, i) >> 24) != OP_INS;
        CHECK(span == ref_len && effective_len_hd(o.ops.data(), n_ops) == ref_len);
    }
    return o;
}
static void expect(const Out& o, const std::vector<uint32_t>& want) {
    CHECK(o.cls == ALN_OK);
    CHECK(o.ops.size() == want.size());
    for (size_t i = 0; i < want.size(); ++i) {
        if (o.ops[i] != want[i]) { std::fprintf(stderr, "operation %zu: %08x, expected %08x\n", i, o.ops[i], want[i]); std::exit(1); }
    }
}

static void tracks_by_hand() {
    const uint32_t M = OP_MATCH, X = OP_MISMATCH, I = OP_INS, D = OP_DEL;
    expect(run("4M", "4", 4, false), {op(M, 0), op(M, 1), op(M, 2), op(M, 3)});
    expect(run("4M", "4", 4, true), {op(M, 0), op(M, 1), op(M, 2), op(M, 3)});
    expect(run("4M", "0A3", 4, false), {op(X, 0, 'A'), op(M, 1), op(M, 2), op(M, 3)});
    expect(run("4M", "A3", 4, false), {op(X, 0, 'A'), op(M, 1), op(M, 2), op(M, 3)});
    expect(run("4M", "0A3", 4, true), {op(M, 0), op(M, 1), op(M, 2), op(X, 3, 'T')});
    expect(run("4M", "3c0", 4, false), {op(M, 0), op(M, 1), op(M, 2), op(X, 3, 'C')});
    expect(run("4M", "3c0", 4, true), {op(X, 0, 'G'), op(M, 1), op(M, 2), op(M, 3)});
    expect(run("5M", "1A0C2", 5, false), {op(M, 0), op(X, 1, 'A'), op(X, 2, 'C'), op(M, 3), op(M, 4)});
    expect(run("5M2D4M", "5^AC0T3", 9, false),
           {op(M, 0), op(M, 1), op(M, 2), op(M, 3), op(M, 4), op(D, 4, 'A'), op(D, 4, 'C'), op(X, 5, 'T'), op(M, 6), op(M, 7), op(M, 8)});
    expect(run("5M2D4M", "5^AC0T3", 9, true),
           {op(M, 0), op(M, 1), op(M, 2), op(X, 3, 'A'), op(D, 3, 'G'), op(D, 3, 'T'), op(M, 4), op(M, 5), op(M, 6), op(M, 7), op(M, 8)});
    expect(run("2M3D2M", "2^acg2", 4, false), {op(M, 0), op(M, 1), op(D, 1, 'A'), op(D, 1, 'C'), op(D, 1, 'G'), op(M, 2), op(M, 3)});
    expect(run("2M2I1D2M", "2^G2", 6, false), {op(M, 0), op(M, 1), op(I, 2), op(I, 3), op(D, 3, 'G'), op(M, 4), op(M, 5)});
    expect(run("2M1D2I2M", "2^G2", 6, false), {op(M, 0), op(M, 1), op(D, 1, 'G'), op(I, 2), op(I, 3), op(M, 4), op(M, 5)});
    expect(run("2=1X1=", "4", 4, false), {op(M, 0), op(M, 1), op(M, 2), op(M, 3)});  // = and X are not trusted over MD
    expect(run("4=", "1N2", 4, false), {op(M, 0), op(X, 1, 'N'), op(M, 2), op(M, 3)});
    expect(run("3M", "0R2", 3, true), {op(M, 0), op(M, 1), op(X, 2, 'Y')});
    expect(run("0M2M0I0D2M", "4", 4, false), {op(M, 0), op(M, 1), op(M, 2), op(M, 3)});
    expect(run("1M", "1", 1, true), {op(M, 0)});
    expect(run("1M", "0g0", 1, true), {op(X, 0, 'C')});
    // a model that starts in the middle of the read (L / 2 = 3): a deletion behind the start carries the position in front of it
    expect(run("1M1D5M", "1^A5", 6, false, false), {op(M, 0), op(D, 0, 'A'), op(M, 1), op(M, 2), op(M, 3), op(M, 4), op(M, 5)});
    expect(run("5M1D1M", "5^A1", 6, false, false), {op(M, 0), op(M, 1), op(M, 2), op(M, 3), op(M, 4), op(D, 5, 'A'), op(M, 5)});
    // the contigs' edges
    CHECK(run("25M", "25", 25, false, true, 0, 3000 - 25).cls == ALN_OK);
    CHECK(run("25M", "0C24", 25, true, true, 1, 0).cr.first.abs == 3000);
    CHECK(run("10M1D5M", "10^A5", 15, false, true, 1, 2000 - 16).cls == ALN_OK);
}

static void long_shapes() {
    for (uint32_t L : {1u, 63u, 64u, 65u, 129u}) {
        for (bool rev : {false, true}) {
            const Out a = run(std::to_string(L) + "M", std::to_string(L), L, rev);
            CHECK(a.cls == ALN_OK);
            for (uint32_t i = 0; i < L; ++i) CHECK(a.ops[i] == op(OP_MATCH, i));
            const Out b = run(std::to_string(L) + "M", std::to_string(L - 1) + "T0", L, rev);  // the last column of the alignment
            CHECK(b.cls == ALN_OK);
            const uint32_t at = rev ? 0 : L - 1;
            for (uint32_t i = 0; i < L; ++i) CHECK(b.ops[i] == (i == at ? op(OP_MISMATCH, i, rev ? 'A' : 'T') : op(OP_MATCH, i)));
        }
    }
    {   // 200 bases of alternating 1M1I: more than 64 CIGAR operations
        std::string c;
        for (int i = 0; i < 100; ++i) c += "1M1I";
        for (bool rev : {false, true}) {
            const Out o = run(c, "100", 200, rev);
            CHECK(o.cls == ALN_OK && o.ops.size() == 200);
            for (uint32_t i = 0; i < 200; ++i) CHECK(o.ops[i] == op(((rev ? 199 - i : i) & 1) ? OP_INS : OP_MATCH, i));
        }
    }
    for (bool rev : {false, true}) {  // a deletion that straddles column 64
        const Out o = run("62M5D30M", "62^ACGTA30", 92, rev);
        CHECK(o.cls == ALN_OK && o.ops.size() == 97);
        uint32_t dels = 0;
        for (uint32_t k = 0; k < 97; ++k) {
            const uint32_t w = coverage_ref_op(o.ops.data(), 97, rev, k);
            CHECK((w >> 24) == (k >= 62 && k < 67 ? (uint32_t)OP_DEL : (uint32_t)OP_MATCH));
            dels += (w >> 24) == OP_DEL;
            if ((w >> 24) == OP_DEL) CHECK(((w >> 16) & 0xFF) == (uint32_t)(rev ? complement_hd("ACGTA"[k - 62]) : "ACGTA"[k - 62]) && (w & 0xFFFF) == (rev ? 29u : 61u));
        }
        CHECK(dels == 5);
    }
}

static void classes() {
    // each with faults of later classes too: the class is the first that applies
    CHECK(run("10M", "", 10, false, true, 0, 100, 0x4, 0, 10).cls == ALN_UNMAPPED);
    CHECK(run("10M", "10", 10, false, true, -1).cls == ALN_UNMAPPED);
    CHECK(run("10M", "10", 10, false, true, 0, -1).cls == ALN_UNMAPPED);
    CHECK(run("5S5M", "", 10, false, true, 9, 100, 0, 5, 10).cls == ALN_BELOW_MIN_MAPQ);
    CHECK(run("5S5M", "", 10, false, true, 9, 100, 0, 10, 10).cls == ALN_NO_MD);
    CHECK(run("5S5M", "7", 12, false, true, 2).cls == ALN_BAD_CONTIG);
    CHECK(run("5S5M", "7", 12, false).cls == ALN_UNSUPPORTED_CIGAR);
    CHECK(run("5H10M", "10", 10, false).cls == ALN_UNSUPPORTED_CIGAR);
    CHECK(run("5M100N5M", "10", 10, false).cls == ALN_UNSUPPORTED_CIGAR);
    CHECK(run("5M1P5M", "10", 10, false).cls == ALN_UNSUPPORTED_CIGAR);
    CHECK(run("", "10", 10, false).cls == ALN_UNSUPPORTED_CIGAR);
    CHECK(run("10M", "9", 12, false, true, 0, 2995).cls == ALN_LENGTH_MISMATCH);
    CHECK(run("5M2I5M", "10", 10, false).cls == ALN_LENGTH_MISMATCH);
    CHECK(run("10M", "9", 10, false, true, 0, 2995).cls == ALN_MD_MISMATCH);
    CHECK(run("10M", "11", 10, false).cls == ALN_MD_MISMATCH);
    CHECK(run("10M", "4^A5", 10, false).cls == ALN_MD_MISMATCH);
    CHECK(run("5M1D5M", "11", 10, false).cls == ALN_MD_MISMATCH);
    CHECK(run("5M1D5M", "5A5", 10, false).cls == ALN_MD_MISMATCH);
    CHECK(run("10M", "5?4", 10, false).cls == ALN_MD_MISMATCH);
    CHECK(run("10M", "5^5", 10, false).cls == ALN_MD_MISMATCH);
    CHECK(run("10M", "10^", 10, false).cls == ALN_MD_MISMATCH);
    CHECK(run("10M", "00000000010", 10, false).cls == ALN_MD_MISMATCH);
    CHECK(run("10M", "0000000010", 10, false).cls == ALN_OK);
    CHECK(run("10M", "70000", 10, false).cls == ALN_MD_MISMATCH);
    CHECK(run("10M", "10", 10, false, true, 0, 2995).cls == ALN_OFF_CONTIG);
    CHECK(run("5M1D5M", "5^A5", 10, false, true, 0, 2990).cls == ALN_OFF_CONTIG);
    CHECK(run("5M1D5M", "5^A5", 10, false, true, 0, 2989).cls == ALN_OK);
    CHECK(run("10M", "10", 10, false, true, 0, 3000).cls == ALN_OFF_CONTIG);
    CHECK(run("10M", "10", 10, false, true, 0, 100, 0, 30, 30).cls == ALN_OK);
    CHECK(run("10M", "10", 10, false, true, 0, 100, 0, 29, 30).cls == ALN_BELOW_MIN_MAPQ);
    CHECK(run("10M", "10", 10, false, true, 0, 100, 0, 37, 0, 0).h.size == 1);  // no X0 tag
}

// the lane-parallel reading of MD — every byte says what it adds to the reference offset, looking only at its neighbours — sums to what the serial reader walks
static void md_bytes_against_the_serial_reader() {
    for (const char* s : {"50", "0A29", "10A0C5", "5^AC0T3", "20^ACG20", "0", "00", "12^a0c0^GT0", "1A1C1G1T1", "007", "65535", "9^ACGTACGTACGT9"}) {
        const std::string str(s);
        const std::vector<uint8_t> md(str.begin(), str.end());
        uint64_t sum = 0;
        bool bad = false;
        for (uint32_t i = 0; i < md.size(); ++i) sum += align_md_advance(md.data(), (uint32_t)md.size(), i, bad);
        AlignMd m = align_md_open(md.data(), (uint32_t)md.size());
        uint64_t walked = 0, deleted = 0;
        for (uint32_t r; (r = align_md_next(m)) != kAlignMdEnd;) { walked += 1; deleted += (r & kAlignDeleted) != 0; }
        CHECK(!bad && !m.bad && sum == walked);
        uint64_t carets = 0;
        for (uint8_t c : md) carets += c == '^';
        CHECK((deleted > 0) == (carets > 0));
    }
    for (const char* s : {"5?4", "5^5", "10^", "^", "00000000010", "65536", "5 5"}) {
        const std::string str(s);
        const std::vector<uint8_t> md(str.begin(), str.end());
        bool bad = false;
        for (uint32_t i = 0; i < md.size(); ++i) (void)align_md_advance(md.data(), (uint32_t)md.size(), i, bad);
        AlignMd m = align_md_open(md.data(), (uint32_t)md.size());
        while (align_md_next(m) != kAlignMdEnd) {}
        CHECK(bad && m.bad);
    }
}

int main() {
    tracks_by_hand();
    long_shapes();
    classes();
    md_bytes_against_the_serial_reader();
    std::printf("align selftest ok\n");
    return 0;
}
