// panel_selftest.cpp — the SNP panel of mapad_amd/csrc/panel_core.hpp driven directly on the host: the 64-probe search at the sizes where its rounds change,
// the walk's windows of 64 slots and trips of 64 operations on reads that hold more slots than a window, the strand axis, the text's end, and the call rule at
// its edges.  A stand-alone program (tests/test_panel_host.py builds it with -fsanitize=address,undefined and runs it as a child process); exits 0 and prints
// "panel selftest ok" when every check holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../mapad_amd/csrc/panel_core.hpp"

using namespace mapad;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static uint32_t op(uint32_t kind, uint32_t read_pos) { return kind << 24 | (uint32_t)'A' << 16 | read_pos; }

struct Acc {
    uint64_t S;
    std::vector<uint64_t> slot_x;  // exact-size heap copies: the sanitizer sees a read or a write beyond them
    std::vector<uint32_t> counts;
    unsigned long long scalars[PAN_SCALARS] = {};
    Acc(uint64_t s, std::vector<uint64_t> x) : S(s), slot_x(std::move(x)), counts(slot_x.size() * kPanelCell, 0) {}
    uint32_t at(uint64_t slot, uint32_t strand, uint32_t b) const { return counts[(slot * 2 + strand) * 4 + b]; }
    uint64_t total() const { uint64_t t = 0; for (uint32_t v : counts) t += v; return t; }
};
// one mapped read with the given track (in track order) at absolute position abs
static bool add(Acc& A, const std::vector<uint32_t>& ops, const std::string& read, uint64_t abs, bool backward, PileupFilter F = PileupFilter{0, 0, 0}, uint8_t qual = 40,
                int mode = 1, uint64_t x0 = 1, bool skip = false) {
    HitRec h{};
    h.n_ops = (uint32_t)ops.size(); h.ops_off = 0;
    CoordRec cr{};
    cr.mapped = 1; cr.error = 0; cr.x0 = x0; cr.best = 0; cr.first.abs = abs; cr.first.backward = backward ? 1 : 0;
    std::vector<uint8_t> r(read.begin(), read.end()), q(read.size(), qual);
    return panel_read(cr, &h, ops.data(), r.data(), q.data(), (uint32_t)r.size(), mode, F, A.S, A.slot_x.data(), A.slot_x.size(), A.counts.data(), A.scalars, skip);
}
// a forward read of n matches, read position i at column i
static std::vector<uint32_t> matches(uint32_t n) { std::vector<uint32_t> t; for (uint32_t i = 0; i < n; ++i) t.push_back(op(OP_MATCH, i)); return t; }

static uint8_t call_of(const uint32_t* cell, char ref, char alt, PanelRule R, uint64_t i, unsigned long long* w = nullptr, uint32_t slot = 0) {
    return panel_call_row(slot, cell, (uint8_t)ref, (uint8_t)alt, R, i, w);
}

int main() {
    {   // the search: sizes around a round's 64 probes and beyond two rounds; targets before, on, between and behind the slots
        for (uint64_t n : {0ull, 1ull, 2ull, 63ull, 64ull, 65ull, 127ull, 128ull, 129ull, 4095ull, 4096ull, 4097ull, 262145ull}) {
            std::vector<uint64_t> x(n);
            for (uint64_t i = 0; i < n; ++i) x[i] = 10 + 3 * i + (i % 7 == 0);  // ascending, distinct, gaps of 2 to 4
            std::vector<uint64_t> exact(x);                                     // (heap, exact size)
            uint32_t most = 0;
            const auto check = [&](uint64_t target) {
                uint32_t rounds = 0;
                const uint64_t got = panel_lower_bound(exact.data(), n, target, &rounds);
                CHECK(got == (uint64_t)(std::lower_bound(x.begin(), x.end(), target) - x.begin()));
                most = std::max(most, rounds);
            };
            check(0); check(9); check(10); check(11); check(~0ull);
            if (n) { check(x[n - 1] - 1); check(x[n - 1]); check(x[n - 1] + 1); }
            const uint64_t stride = n > 5000 ? 97 : 1;
            for (uint64_t i = 0; i < n; i += stride) { check(x[i] - 1); check(x[i]); check(x[i] + 1); }
            uint32_t bound = 0;  // ceil(log64 n) rounds, and one more where n is a power of 64 (the last probe of a chunk is not looked at again, the first is)
            for (uint64_t m = 1; m <= n; m *= 64) ++bound;
            CHECK(most <= bound);
            if (n == 0) CHECK(most == 0);
        }
    }
    {   // 130 slots inside one read of 150 matches: three windows, three trips; every column on its own slot, both strands
        std::vector<uint64_t> x;
        for (uint64_t i = 0; i < 130; ++i) x.push_back(1000 + 10 + i);  // slots on columns 10 .. 139
        x.insert(x.begin(), {5, 400, 999});
        x.push_back(1150); x.push_back(1151); x.push_back(5000);        // slots before and directly behind the read
        std::string read(150, 'A');
        for (uint32_t i = 0; i < 150; ++i) read[i] = "ACGT"[i & 3];
        Acc A(6000, x);
        CHECK(add(A, matches(150), read, 1000, false));
        CHECK(A.scalars[PAN_READS] == 1 && A.scalars[PAN_ON_PANEL] == 1 && A.scalars[PAN_COUNTED] == 130 && A.total() == 130);
        for (uint32_t i = 0; i < 130; ++i) CHECK(A.at(3 + i, 0, (10 + i) & 3) == 1);
        CHECK(A.at(2, 0, 0) + A.at(2, 0, 1) + A.at(2, 0, 2) + A.at(2, 0, 3) == 0 && A.at(133, 0, 2) == 0);  // 999 and 1150 lie outside [1000, 1150)
        // the same read reported on the reverse strand: track order reversed, read position p at column 149 - p, bases complemented, strand 1
        std::vector<uint32_t> back;
        for (uint32_t p = 0; p < 150; ++p) back.push_back(op(OP_MATCH, p));
        CHECK(add(A, back, read, 1000, true));
        for (uint32_t i = 0; i < 130; ++i) CHECK(A.at(3 + i, 1, 3 - ((149 - (10 + i)) & 3)) == 1 && A.at(3 + i, 0, (10 + i) & 3) == 1);
        CHECK(A.scalars[PAN_COUNTED] == 260 && A.total() == 260);
    }
    {   // insertions shift read positions, deletions shift columns; a deleted slot counts as such only; a trip boundary inside the gaps
        std::vector<uint64_t> x = {100, 131, 132, 133, 170, 199, 200};
        Acc A(1000, x);
        std::vector<uint32_t> t;
        std::string read;
        uint32_t p = 0;
        for (uint32_t i = 0; i < 30; ++i) { t.push_back(op(OP_MATCH, p++)); read += 'C'; }   // columns 100 .. 129
        for (uint32_t i = 0; i < 5; ++i) { t.push_back(op(OP_INS, p++)); read += 'T'; }      // no column
        t.push_back(op(OP_MATCH, p++)); read += 'G';                                         // column 130
        t.push_back(op(OP_DEL, p)); t.push_back(op(OP_DEL, p));                              // columns 131, 132: deleted
        for (uint32_t i = 0; i < 67; ++i) { t.push_back(op(OP_MATCH, p++)); read += (i == 0 ? 'T' : i == 37 ? 'N' : 'A'); }  // columns 133 .. 199; 170 holds an N
        CHECK(t.size() == 105 && read.size() == p);
        CHECK(add(A, t, read, 100, false));
        CHECK(A.scalars[PAN_DELETED] == 2 && A.scalars[PAN_NOT_ACGT] == 1 && A.scalars[PAN_COUNTED] == 3 && A.total() == 3);
        CHECK(A.at(0, 0, 1) == 1 && A.at(3, 0, 3) == 1 && A.at(5, 0, 0) == 1 && A.at(6, 0, 0) == 0);
        // filters: the first three and the last two bases masked, quality below the threshold
        Acc B(1000, x);
        CHECK(add(B, t, read, 100, false, PileupFilter{0, 3, 2}));
        CHECK(B.scalars[PAN_MASKED] == 2 && B.scalars[PAN_COUNTED] == 1 && B.at(3, 0, 3) == 1);  // column 100 (p = 0) and column 199 (the last base)
        Acc C(1000, x);
        CHECK(add(C, t, read, 100, false, PileupFilter{41, 0, 0}));
        CHECK(C.scalars[PAN_LOW_QUAL] == 3 && C.scalars[PAN_NOT_ACGT] == 1 && C.total() == 0);
    }
    {   // reads that count or not; reads off the panel; the text's end
        std::vector<uint64_t> x = {0, 50, 999};
        Acc A(1000, x);
        const std::string read(20, 'G');
        CHECK(add(A, matches(20), read, 0, false) && A.at(0, 0, 2) == 1);                      // on the text's first base
        CHECK(add(A, matches(20), read, 980, false) && A.at(2, 0, 2) == 1);                    // ... and its last
        CHECK(add(A, matches(20), read, 51, false) && add(A, matches(20), read, 30, false));   // between slots; slot 50 is one behind the read's last column
        CHECK(A.scalars[PAN_READS] == 4 && A.scalars[PAN_ON_PANEL] == 2 && A.total() == 2);
        CHECK(add(A, matches(20), read, 40, false, PileupFilter{0, 0, 0}, 40, 2, 2) && add(A, matches(20), read, 40, false, PileupFilter{0, 0, 0}, 40, 1, 1, true));
        CHECK(A.scalars[PAN_READS_SEEN] == 6 && A.scalars[PAN_READS] == 4 && A.total() == 2);  // X0 == 2 under mode 2; a read left out: seen, not counted
        CHECK(!add(A, matches(20), read, 981, false) && !add(A, matches(20), read, 1001, false) && A.total() == 2 && A.scalars[PAN_READS] == 4);  // leaves the text
        Acc E(1000, {});
        CHECK(add(E, matches(20), read, 10, false) && E.scalars[PAN_READS] == 1 && E.scalars[PAN_ON_PANEL] == 0);  // a panel of no slots
    }
    {   // the call rule
        const PanelRule draw{0, 1, 0, 7}, major{1, 1, 0, 7};
        uint32_t cell[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        CHECK(call_of(cell, 'A', 'C', draw, 0) == '9');                                         // n = 0
        CHECK(call_of(cell, 'A', 'C', draw, 0, nullptr, kPanelNoSlot) == '9');
        cell[0] = 2; cell[4 + 1] = 1;                                                           // two A forward, one C reverse
        CHECK(call_of(cell, 'A', 'C', PanelRule{0, 3, 0, 7}, 0) != '9' && call_of(cell, 'A', 'C', PanelRule{0, 4, 0, 7}, 0) == '9');  // min_depth exactly, and one above
        CHECK(call_of(cell, 'A', 'C', major, 0) == '2' && call_of(cell, 'C', 'A', major, 0) == '0' && call_of(cell, 'a', 'c', major, 0) == '2');
        CHECK(call_of(cell, 'A', 'A', major, 0) == '9' && call_of(cell, 'N', 'A', major, 0) == '9' && call_of(cell, 'A', '-', major, 0) == '9');
        CHECK(call_of(cell, 'G', 'T', major, 0) == '9');                                        // observed, but neither allele
        // only ref or only alt observed: the draw has no choice
        for (uint64_t i = 0; i < 2000; ++i) { CHECK(call_of(cell, 'A', 'G', draw, i) == '2'); CHECK(call_of(cell, 'G', 'A', draw, i) == '0'); }
        // a tie under the majority rule is the draw: both outcomes occur over the rows, each row's is what the draw says
        cell[0] = 5; cell[4 + 1] = 5;
        uint32_t refs = 0;
        for (uint64_t i = 0; i < 2000; ++i) {
            const uint8_t m = call_of(cell, 'A', 'C', major, i), d = call_of(cell, 'A', 'C', draw, i);
            CHECK(m == d && (m == '2' || m == '0'));
            CHECK((d == '2') == (panel_mulhi(panel_mix(7, i), 10) < 5));
            refs += d == '2';
        }
        CHECK(refs > 800 && refs < 1200);  // 2000 fair draws: 1000 +- 22 (one standard deviation)
        CHECK(panel_mix(0, 0) == 0xE220A8397B1DCDAFull);  // splitmix64's first output for seed 0
        CHECK(panel_mulhi(~0ull, ~0ull) == ~0ull - 1 && panel_mulhi(1ull << 63, 2) == 1 && panel_mulhi(12345, 0) == 0);
        // transitions: missing under 1; the documented strand under 2
        uint32_t ct[8] = {0, 3, 0, 9, 0, 4, 0, 0};  // forward: 3 C, 9 T (damage); reverse: 4 C
        unsigned long long w[PANS_WORDS] = {};
        CHECK(call_of(ct, 'C', 'T', PanelRule{1, 1, 0, 1}, 0) == '0' && call_of(ct, 'C', 'T', PanelRule{1, 1, 1, 1}, 0) == '9');
        CHECK(call_of(ct, 'C', 'T', PanelRule{1, 1, 2, 1}, 0, w) == '2' && call_of(ct, 'T', 'C', PanelRule{1, 1, 2, 1}, 0) == '0');  // reverse strand only: 4 C
        CHECK(w[PANS_ROWS] == 1 && w[PANS_TRANSITION] == 1 && w[PANS_OBS_REF] == 4 && w[PANS_OBS_ALT] == 0 && w[PANS_MAX_DEPTH] == 4 && w[PANS_TRANSITIONS_CALLED] == 1);
        uint32_t ga[8] = {2, 0, 0, 0, 7, 0, 1, 0};  // forward: 2 A; reverse: 7 A (damage), 1 G
        CHECK(call_of(ga, 'G', 'A', PanelRule{1, 1, 0, 1}, 0) == '0' && call_of(ga, 'G', 'A', PanelRule{1, 1, 2, 1}, 0) == '0');
        CHECK(call_of(ga, 'G', 'A', PanelRule{1, 3, 2, 1}, 0) == '9');                          // forward strand only: 2 < 3
        CHECK(call_of(ga, 'G', 'C', PanelRule{1, 1, 2, 1}, 0) == '2');                          // a transversion uses both strands whatever the setting
        uint32_t big[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0};   // sums beyond 32 bits
        unsigned long long wb[PANS_WORDS] = {};
        (void)call_of(big, 'A', 'C', draw, 3, wb);
        CHECK(wb[PANS_OBS_REF] == 2ull * 0xFFFFFFFFull && wb[PANS_MAX_DEPTH] == 4ull * 0xFFFFFFFFull && wb[PANS_CALLED] == 1);
        CHECK(panel_rule_ok(draw) && !panel_rule_ok(PanelRule{2, 1, 0, 0}) && !panel_rule_ok(PanelRule{0, 0, 0, 0}) && !panel_rule_ok(PanelRule{0, 1, 3, 0}));
    }
    std::printf("panel selftest ok\n");
    return 0;
}
