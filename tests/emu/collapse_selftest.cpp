// collapse_selftest.cpp — TEST-ONLY: the host build of the duplicate grouping (mapad_amd/csrc/collapse_core.hpp) over a whole batch, the way the two kernels
// of mapad_amd.hip run it: an insert pass (key from the four lanes' shares, table insert) and a match pass (table lookup, byte compare by four lanes, who
// represents whom).  `key_bits` cuts the key down so that most candidates collide: the path real 64-bit keys never take in a test.
// Built by tests/test_collapse_host.py; never loaded by the product.
#include <cstdint>
#include <vector>

#include "../../mapad_amd/csrc/collapse_core.hpp"

using namespace mapad;

namespace {
struct HostAtomics {
    static uint64_t cas64(uint64_t* p, uint64_t expected, uint64_t desired) { const uint64_t old = *p; if (old == expected) *p = desired; return old; }
    static void max32(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
};
}  // namespace

extern "C" {

// dup_of[n_reads]; stats = {groups, reads that had a twin, collisions kept apart by the byte compare}.  Returns 0, or 1 on a broken invariant.
int collapse_group_host(const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint32_t n_reads, int ignore_qual, int key_bits, uint32_t* dup_of, uint64_t* stats) {
    uint64_t slots = 64;
    while (slots < 2 * (uint64_t)n_reads) slots <<= 1;
    std::vector<uint64_t> keys(slots, 0), read_key(n_reads, 0);
    std::vector<uint32_t> inv(slots, 0), has_dup(n_reads, 0);
    const collapse::Table tab{keys.data(), inv.data(), slots - 1};
    for (uint32_t i = 0; i < n_reads; ++i) {
        const uint64_t off = offsets[i];
        const int L = (int)(offsets[i + 1] - off);
        uint64_t sum = 0;
        for (int w = 0; w < 4; ++w) sum += collapse::key_partial(seqs + off, quals + off, L, ignore_qual != 0, w, 4);
        read_key[i] = collapse::key_finish(sum, L, key_bits);
        collapse::table_insert<HostAtomics>(tab, read_key[i], i);
    }
    stats[0] = stats[1] = stats[2] = 0;
    for (uint32_t i = 0; i < n_reads; ++i) {
        const uint32_t cand = collapse::table_find(tab, read_key[i], i);
        bool same = true;
        if (cand != i) {
            const uint64_t off = offsets[i], off_c = offsets[cand];
            const int L = (int)(offsets[i + 1] - off);
            same = (int)(offsets[cand + 1] - off_c) == L;
            for (int w = 0; w < 4 && same; ++w) same = collapse::equal_partial(seqs + off, quals + off, seqs + off_c, quals + off_c, L, ignore_qual != 0, w, 4);
        }
        const uint32_t rep = collapse::representative(i, cand, same);
        if (rep > i) return 1;
        dup_of[i] = rep;
        if (rep != i) { if (!has_dup[rep]) { has_dup[rep] = 1; stats[1] += 1; } stats[1] += 1; }
        else { stats[0] += 1; if (cand != i) stats[2] += 1; }
    }
    return 0;
}

}  // extern "C"
