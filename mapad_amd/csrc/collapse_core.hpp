// collapse_core.hpp — per-read logic of duplicate collapsing: which reads of a batch are byte-for-byte the same read, and which of them is mapped.
//
// A group is a set of reads of one batch with equal length, equal bases and — unless the parameters ignore base qualities — equal qualities; its
// representative is the member with the lowest read index.  Two passes over the batch, one quad per read (mapad_amd.hip: collapse_insert_kernel,
// collapse_match_kernel):
//   insert : a 64-bit key over length, bases and qualities; the key is entered into an open-addressing table in HBM (compare-and-swap on the key
//            word, linear probing) and the table keeps the lowest read index seen under that key (stored complemented, so that an all-zero table
//            is an empty one and "lowest index" is an atomic max);
//   match  : the read looks its key up, finds the candidate representative and compares its own bytes with the candidate's.  Only equal bytes
//            make a duplicate: a read whose key collides with another read's is mapped on its own (the collision costs a collapse, never a result).
// The key is a SUM of per-chunk terms (four bases + four qualities each), so the lanes of a quad each take every fourth chunk and add up.
// Written like search_core.hpp: plain C++ that g++ compiles for the host as well (tests/emu/collapse_selftest.cpp runs these very functions
// against an independent grouping); the atomics come in through a policy type.
#pragma once
#include "common.hpp"

namespace mapad {
namespace collapse {

MAPAD_HD uint64_t mix64(uint64_t x) {  // splitmix64's finaliser
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// bytes [0, min(n, 4)) at p as a little-endian word, zero-padded
MAPAD_HD uint32_t load4(const uint8_t* p, int n) {
    uint32_t v = 0;
    if (n >= 4) { __builtin_memcpy(&v, p, 4); return v; }
    for (int k = 0; k < n; ++k) v |= (uint32_t)p[k] << (8 * k);
    return v;
}

// this lane's share of the key of read (seq, qual, L): chunks lane, lane + n_lanes, ... of four positions each.  The shares of all lanes add up (mod 2^64).
MAPAD_HD uint64_t key_partial(const uint8_t* seq, const uint8_t* qual, int L, bool ignore_qual, int lane, int n_lanes) {
    uint64_t sum = 0;
    for (int c = lane; 4 * c < L; c += n_lanes) {
        uint64_t v = load4(seq + 4 * c, L - 4 * c);
        if (!ignore_qual) v |= (uint64_t)load4(qual + 4 * c, L - 4 * c) << 32;
        sum += mix64(v + mix64((uint64_t)c + 1));
    }
    return sum;
}
// the key from the summed shares.  key_bits < 64 cuts it down (test hook: most candidates then collide); 0 is the table's "empty" and never a key.
MAPAD_HD uint64_t key_finish(uint64_t sum, int L, int key_bits = 64) {
    uint64_t key = mix64(sum ^ ((uint64_t)L * 0xD6E8FEB86659FD93ull));
    if (key_bits < 64) key &= (1ull << key_bits) - 1;
    return key ? key : 1;
}

// this lane's share of "reads a and b of equal length L are the same read": all lanes' answers are ANDed
MAPAD_HD bool equal_partial(const uint8_t* seq_a, const uint8_t* qual_a, const uint8_t* seq_b, const uint8_t* qual_b, int L, bool ignore_qual, int lane, int n_lanes) {
    bool same = true;
    for (int c = lane; 4 * c < L; c += n_lanes) {
        same &= load4(seq_a + 4 * c, L - 4 * c) == load4(seq_b + 4 * c, L - 4 * c);
        if (!ignore_qual) same &= load4(qual_a + 4 * c, L - 4 * c) == load4(qual_b + 4 * c, L - 4 * c);
    }
    return same;
}

// open addressing, linear probing; `mask` + 1 slots, a power of two of at least twice the batch's reads, all zero before the first insert
struct Table {
    uint64_t* keys;     // 0 = empty
    uint32_t* inv_min;  // ~(lowest read index entered under the slot's key); 0 = none yet
    uint64_t mask;
};
// At::cas64(p, expected, desired) -> old value; At::max32(p, v)
template <class At>
MAPAD_HD void table_insert(const Table& t, uint64_t key, uint32_t read) {
    for (uint64_t s = key & t.mask;; s = (s + 1) & t.mask) {
        const uint64_t old = At::cas64(&t.keys[s], 0ull, key);
        if (old == 0 || old == key) { At::max32(&t.inv_min[s], ~read); return; }
    }
}
// the lowest read index entered under `key` (every read of the batch has been inserted: the key is there; `read` itself if it were not)
MAPAD_HD uint32_t table_find(const Table& t, uint64_t key, uint32_t read) {
    for (uint64_t s = key & t.mask;; s = (s + 1) & t.mask) {
        const uint64_t k = t.keys[s];
        if (k == key) return ~t.inv_min[s];
        if (k == 0) return read;
    }
}
// who is searched for read `read`: the candidate if the bytes are the same, else the read itself
MAPAD_HD uint32_t representative(uint32_t read, uint32_t candidate, bool same_bytes) { return (candidate != read && same_bytes) ? candidate : read; }

}  // namespace collapse
}  // namespace mapad
