// dedup_core.hpp — PCR duplicates by alignment coordinates: which of the reads a run reports are copies of a fragment that an earlier read already showed.
// The step an ancient-DNA pipeline runs between mapping and everything that counts (damage, coverage, genotypes), taken from what is on the device after a
// batch anyway — the records kernel's CoordRec and the reported alignment's edit track — instead of from a coordinate sort of the BAM and an external tool.
// One source for the dedup_* kernels (mapad_amd.hip), the host path (mapad_dedup_host_*) and tests/emu/dedup_selftest.cpp; the atomics come in through a
// policy type, as in collapse_core.hpp.
//
// Definition.  A read is eligible iff cr.mapped && !cr.error (whatever the mode of the other analyses, whatever X0).  Its key is the triple
// (cr.first.abs, eff, cr.first.backward), eff = effective_len_hd of the track of hits[cr.best]: both ends of the fragment and the strand.  Merged and
// single-end ancient reads are whole fragments, so the same start with another end is another molecule; the same span under another CIGAR (an insertion) is a
// duplicate, a deletion changes eff and is none.  The key is exact, not a hash: key = ((abs << 23) | (eff << 1) | backward) + 1 with abs < 2^40 and
// eff < 2^22, so it fits 64 bits, 0 stays free for "empty slot", and there is neither a byte comparison nor a false duplicate.  Every read has a global
// ordinal: the reads of the batches marked before its own, plus its index in its batch.  Of all eligible reads seen so far under one key the one with the
// lowest ordinal is the original, every other one a duplicate: "first in input order wins", which can be decided while the output is streamed and does not
// depend on how the input is cut into batches.  Reads from repeats take the coordinate the seeded draw gives them.
//
// Table.  Open addressing, linear probing, a power-of-two number of slots, home slot mix64(key) & mask.  A slot is 32 bytes — key, ~ordinal of the lowest
// ordinal seen (kept by atomic max, so a zeroed table is an empty one), member count — and 32-byte aligned: the three words a probe touches lie in one
// 64-byte line, and so does the neighbour a collision moves on to every second time.  The host keeps 2 * (entries + reads of the next batch) <= slots, so a
// probe sequence ends; the loops are bounded by the table's size all the same and report a full table instead of spinning.
#pragma once
#include <vector>

#include "collapse_core.hpp"
#include "coverage_core.hpp"

namespace mapad {
namespace dedup {

constexpr uint32_t kBins = 256;  // MAPAD_DUPLICATES_BINS: histogram of member counts, bin k = fragments seen k times, the last bin is >= 255
constexpr uint64_t kAbsLimit = 1ull << 40, kEffLimit = 1ull << 22;
constexpr uint64_t kMinSlots = 8;
enum : uint32_t { DD_READS_SEEN = 0, DD_ELIGIBLE, DD_DUPLICATES, DD_FRAGMENTS, DD_SCALARS };
enum : int { kFull = -1, kFound = 0, kClaimed = 1 };

struct alignas(32) Slot {
    uint64_t key;      // 0 = empty
    uint64_t inv_ord;  // ~(lowest ordinal entered under the key)
    uint32_t count;    // members entered under the key
    uint32_t pad[3];
};
static_assert(sizeof(Slot) == 32, "two slots per 64-byte line");
struct Table { Slot* slots; uint64_t mask; };  // mask + 1 slots

MAPAD_HD bool eligible(uint32_t mapped, uint32_t error) { return mapped && !error; }
// false: the coordinate does not fit the packing (never from record_coords on a text the context accepts)
MAPAD_HD bool make_key(uint64_t abs, uint64_t eff, bool backward, uint64_t& key) {
    if (abs >= kAbsLimit || eff >= kEffLimit) return false;
    key = ((abs << 23) | (eff << 1) | (backward ? 1ull : 0ull)) + 1;
    return true;
}
// the key of one eligible read; hits = the read's hit records
MAPAD_HD bool read_key(const CoordRec& cr, const HitRec* hits, const uint32_t* ops, uint64_t& key) {
    const HitRec& h = hits[cr.best];
    return make_key(cr.first.abs, effective_len_hd(ops + h.ops_off, h.n_ops), cr.first.backward != 0, key);
}
MAPAD_HD uint32_t hist_bin(uint32_t count) { return count >= kBins - 1 ? kBins - 1 : count; }
// the smallest power-of-two table that keeps 2 * fragments <= slots
MAPAD_HD uint64_t slots_for(uint64_t fragments) {
    uint64_t s = kMinSlots;
    while (s < 2 * fragments) s <<= 1;
    return s;
}

// At::cas64(p, expected, desired) -> old value; At::max64(p, v); At::add32(p, v).  Enters `count` members with lowest ordinal ~inv_ord under `key`:
// kClaimed (the key is new), kFound, or kFull (no free slot in mask + 1 probes; nothing entered).
template <class At>
MAPAD_HD int table_insert(const Table& t, uint64_t key, uint64_t inv_ord, uint32_t count) {
    uint64_t s = collapse::mix64(key) & t.mask;
    for (uint64_t probes = 0; probes <= t.mask; ++probes, s = (s + 1) & t.mask) {
        const uint64_t old = At::cas64(&t.slots[s].key, 0ull, key);
        if (old == 0 || old == key) {
            At::max64(&t.slots[s].inv_ord, inv_ord);
            At::add32(&t.slots[s].count, count);
            return old == 0 ? kClaimed : kFound;
        }
    }
    return kFull;
}
// the slot of `key`, or nullptr (not entered)
MAPAD_HD const Slot* table_find(const Table& t, uint64_t key) {
    uint64_t s = collapse::mix64(key) & t.mask;
    for (uint64_t probes = 0; probes <= t.mask; ++probes, s = (s + 1) & t.mask) {
        const uint64_t k = t.slots[s].key;
        if (k == key) return &t.slots[s];
        if (k == 0) return nullptr;
    }
    return nullptr;
}
// is the read with this ordinal a duplicate?  (after every read of its batch has been entered)
MAPAD_HD bool is_duplicate(const Slot& s, uint64_t ordinal) { return ~s.inv_ord != ordinal; }
// one occupied slot of an old table into a new one: key, ordinal and count survive
template <class At>
MAPAD_HD int rehash_slot(const Table& dst, const Slot& s) { return s.key ? table_insert<At>(dst, s.key, s.inv_ord, s.count) : (int)kFound; }

// ---- the table on the host (one thread): the host path and the self-test ------------------------------------------------------------------
struct HostAtomics {
    static uint64_t cas64(uint64_t* p, uint64_t expected, uint64_t desired) { const uint64_t old = *p; if (old == expected) *p = desired; return old; }
    static void max64(uint64_t* p, uint64_t v) { if (v > *p) *p = v; }
    static void add32(uint32_t* p, uint32_t v) { *p += v; }
};
struct HostTable {
    std::vector<Slot> slots;
    uint64_t entries = 0, grows = 0;
    Table view() { return Table{slots.data(), (uint64_t)slots.size() - 1}; }
    void init(uint64_t n_slots) { slots.assign(slots_for((n_slots + 1) / 2), Slot{}); entries = 0; grows = 0; }
    // room for `more` further keys: 2 * (entries + more) <= slots, or a table of at least twice the size with every occupied slot entered again
    bool reserve(uint64_t more) {
        if (slots.empty()) { slots.assign(slots_for(more), Slot{}); return true; }
        if (2 * (entries + more) <= (uint64_t)slots.size()) return true;
        uint64_t want = slots_for(entries + more);
        if (want < 2 * (uint64_t)slots.size()) want = 2 * (uint64_t)slots.size();
        std::vector<Slot> old(want, Slot{});
        old.swap(slots);
        const Table t = view();
        for (const Slot& s : old) if (rehash_slot<HostAtomics>(t, s) == kFull) return false;
        grows += 1;
        return true;
    }
    int insert(uint64_t key, uint64_t ordinal) {
        const int rc = table_insert<HostAtomics>(view(), key, ~ordinal, 1u);
        entries += rc == kClaimed;
        return rc;
    }
    void histogram(uint64_t* bins) const {  // bins[kBins], added to
        for (const Slot& s : slots) if (s.key) bins[hist_bin(s.count)] += 1;
    }
};

// One batch on one thread (the host path): keys[r] = the read's key or 0 (ineligible), entered under ordinal0 + r; then flags[r] = duplicate.  scalars[DD_*]
// are added to.  false: a coordinate that does not fit the key, or a full table (never with reserve() before).
template <typename KeyOf>
inline bool mark_batch(HostTable& T, uint64_t n, uint64_t ordinal0, KeyOf key_of, uint8_t* flags, uint64_t* scalars) {
    if (!T.reserve(n)) return false;
    std::vector<uint64_t> keys(n, 0);
    for (uint64_t r = 0; r < n; ++r) {
        bool is_eligible = false;
        if (!key_of(r, is_eligible, keys[r])) return false;
        if (!is_eligible) { keys[r] = 0; continue; }
        const int rc = T.insert(keys[r], ordinal0 + r);
        if (rc == kFull) return false;
        scalars[DD_FRAGMENTS] += rc == kClaimed;
    }
    const Table t = T.view();
    for (uint64_t r = 0; r < n; ++r) {
        scalars[DD_READS_SEEN] += 1;
        uint8_t dup = 0;
        if (keys[r]) {
            const Slot* s = table_find(t, keys[r]);
            if (!s) return false;
            dup = is_duplicate(*s, ordinal0 + r);
            scalars[DD_ELIGIBLE] += 1; scalars[DD_DUPLICATES] += dup;
        }
        if (flags) flags[r] = dup;
    }
    return true;
}

}  // namespace dedup
}  // namespace mapad
