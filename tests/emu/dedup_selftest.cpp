// dedup_selftest.cpp — the duplicate table of mapad_amd/csrc/dedup_core.hpp driven directly on the host: the insert, find and rehash functions the dedup_*
// kernels compile, under the host's atomics policy, against a std::map.  A stand-alone program (tests/test_dedup_host.py builds it with
// -fsanitize=address,undefined and runs it as a child process); exits 0 and prints "dedup selftest ok" when every check holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../../mapad_amd/csrc/dedup_core.hpp"

using namespace mapad;
using namespace mapad::dedup;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

struct Want { uint64_t first; uint32_t count; };

// every key of `want` is in the table with its lowest ordinal and its count, and the table holds nothing else
static void check_table(HostTable& T, const std::map<uint64_t, Want>& want) {
    CHECK(T.entries == want.size());
    CHECK((T.slots.size() & (T.slots.size() - 1)) == 0 && 2 * T.entries <= T.slots.size());
    const Table t = T.view();
    for (const auto& kv : want) {
        const Slot* s = table_find(t, kv.first);
        CHECK(s && s->key == kv.first && ~s->inv_ord == kv.second.first && s->count == kv.second.count);
        CHECK(!is_duplicate(*s, kv.second.first) && is_duplicate(*s, kv.second.first + 1));
    }
    uint64_t occupied = 0, members = 0, hist[kBins] = {};
    for (const Slot& s : T.slots) if (s.key) { occupied += 1; members += s.count; CHECK(want.count(s.key)); }
    CHECK(occupied == want.size());
    T.histogram(hist);
    uint64_t sum = 0;
    for (uint32_t k = 0; k < kBins; ++k) sum += hist[k];
    CHECK(sum == occupied && hist[0] == 0);
    (void)members;
}
static void enter(HostTable& T, std::map<uint64_t, Want>& want, uint64_t key, uint64_t ordinal) {
    CHECK(T.reserve(1));
    const int rc = T.insert(key, ordinal);
    auto it = want.find(key);
    CHECK(rc == (it == want.end() ? kClaimed : kFound));
    if (it == want.end()) want[key] = Want{ordinal, 1};
    else { it->second.count += 1; if (ordinal < it->second.first) it->second.first = ordinal; }
}

int main() {
    // the packing: 0 is never a key, the extremes fit, what does not fit is refused
    uint64_t k0 = 0, k1 = 0, k2 = 0, k3 = 0;
    CHECK(make_key(0, 0, false, k0) && k0 == 1);
    CHECK(make_key(0, 0, true, k1) && k1 == 2);
    CHECK(make_key(kAbsLimit - 1, kEffLimit - 1, true, k2) && k2 == (((kAbsLimit - 1) << 23) | ((kEffLimit - 1) << 1) | 1) + 1 && k2 > k1);
    CHECK(make_key(kAbsLimit - 1, kEffLimit - 1, false, k3) && k3 + 1 == k2);
    CHECK(!make_key(kAbsLimit, 1, false, k3) && !make_key(1, kEffLimit, false, k3));
    {   // distinct triples give distinct keys: both ends and the strand take part
        uint64_t a, b, c, d;
        CHECK(make_key(100, 50, false, a) && make_key(100, 51, false, b) && make_key(100, 50, true, c) && make_key(101, 50, false, d));
        CHECK(a != b && a != c && a != d && b != c && b != d && c != d);
    }
    CHECK(hist_bin(1) == 1 && hist_bin(254) == 254 && hist_bin(255) == 255 && hist_bin(100000) == 255);
    CHECK(slots_for(0) == 8 && slots_for(4) == 8 && slots_for(5) == 16 && slots_for(1000) == 2048);

    {   // a table of 8 slots that grows repeatedly; abs = 0 and the largest legal abs and eff among the keys
        HostTable T;
        T.init(8);
        CHECK(T.slots.size() == 8);
        std::map<uint64_t, Want> want;
        enter(T, want, k0, 0); enter(T, want, k2, 1); enter(T, want, k1, 2); enter(T, want, k2, 3); enter(T, want, k0, 4);
        for (uint64_t i = 0; i < 300; ++i) {
            uint64_t key;
            CHECK(make_key(1000 + i / 3, 40 + i % 3, (i & 1) != 0, key));
            enter(T, want, key, 5 + i);
            if (i % 37 == 0) check_table(T, want);
        }
        CHECK(T.grows >= 5 && T.slots.size() >= 2 * want.size());
        check_table(T, want);
        CHECK(want[k0].first == 0 && want[k0].count == 2 && want[k2].first == 1 && want[k2].count == 2);
    }
    {   // probing that wraps around the last slot: keys whose home is the last slot of a table of 16
        std::vector<Slot> slots(16);
        const Table t{slots.data(), 15};
        std::vector<uint64_t> keys;
        for (uint64_t key = 1; keys.size() < 5; ++key) if ((collapse::mix64(key) & 15) == 15) keys.push_back(key);
        for (size_t i = 0; i < keys.size(); ++i) CHECK(table_insert<HostAtomics>(t, keys[i], ~(uint64_t)(10 + i), 1) == kClaimed);
        CHECK(slots[15].key == keys[0] && slots[0].key == keys[1] && slots[1].key == keys[2] && slots[2].key == keys[3] && slots[3].key == keys[4]);
        for (size_t i = 0; i < keys.size(); ++i) { const Slot* s = table_find(t, keys[i]); CHECK(s && ~s->inv_ord == 10 + i && s->count == 1); }
        CHECK(table_insert<HostAtomics>(t, keys[4], ~(uint64_t)3, 1) == kFound && ~slots[3].inv_ord == 3 && slots[3].count == 2);  // a lower ordinal takes over
        CHECK(table_insert<HostAtomics>(t, keys[4], ~(uint64_t)99, 1) == kFound && ~slots[3].inv_ord == 3 && slots[3].count == 3);  // a higher one does not
        uint64_t absent = 0;
        for (uint64_t key = 1000;; ++key) if ((collapse::mix64(key) & 15) == 15) { absent = key; break; }
        CHECK(table_find(t, absent) == nullptr);
        // a full table is reported, not spun on
        for (uint64_t key = 2000, n = keys.size(); n < 16; ++key) n += table_insert<HostAtomics>(t, key, ~key, 1) == kClaimed;
        CHECK(table_insert<HostAtomics>(t, 999999, ~0ull, 1) == kFull && table_find(t, 999999) == nullptr);
    }
    {   // 10 000 random keys with repeats against a std::map, growth on the way, and one rehash checked slot by slot
        std::mt19937_64 rng(12345);
        HostTable T;
        T.init(64);
        std::map<uint64_t, Want> want;
        std::vector<uint64_t> pool;
        for (int i = 0; i < 3000; ++i) {
            uint64_t key;
            CHECK(make_key(rng() % kAbsLimit, 20 + rng() % 200, (rng() & 1) != 0, key));
            pool.push_back(key);
        }
        std::vector<uint64_t> order(10000);
        for (uint64_t i = 0; i < order.size(); ++i) order[i] = i;
        for (uint64_t i = 0; i < order.size(); ++i) {  // ordinals in a shuffled order: the lowest wins, not the first entered
            std::swap(order[i], order[i + rng() % (order.size() - i)]);
            enter(T, want, pool[rng() % pool.size()], order[i]);
        }
        check_table(T, want);
        CHECK(T.grows >= 4);
        const std::vector<Slot> before = T.slots;
        const uint64_t grows = T.grows;
        CHECK(T.reserve(T.slots.size()));  // forces one rehash
        CHECK(T.grows == grows + 1 && T.slots.size() >= 2 * before.size());
        const Table t = T.view();
        for (const Slot& s : before) if (s.key) { const Slot* n = table_find(t, s.key); CHECK(n && n->inv_ord == s.inv_ord && n->count == s.count); }
        check_table(T, want);
    }
    {   // mark_batch: the same reads in one batch and in three give the same flags; a group of more than 255 members lands in the last bin
        std::vector<uint64_t> keys;
        std::mt19937_64 rng(7);
        for (int i = 0; i < 900; ++i) keys.push_back(i % 5 == 4 ? 0 : 1 + rng() % 150);  // 0: not eligible
        for (int i = 0; i < 300; ++i) keys.push_back(777);
        auto run = [&](const std::vector<size_t>& cuts, std::vector<uint8_t>& flags, uint64_t* scalars, HostTable& T) {
            flags.assign(keys.size(), 9);
            size_t at = 0;
            for (size_t end : cuts) {
                auto key_of = [&](uint64_t r, bool& is_eligible, uint64_t& key) { key = keys[at + r]; is_eligible = key != 0; return true; };
                CHECK(mark_batch(T, end - at, at, key_of, flags.data() + at, scalars));
                at = end;
            }
        };
        std::vector<uint8_t> one, three;
        uint64_t s1[DD_SCALARS] = {}, s3[DD_SCALARS] = {};
        HostTable T1, T3;
        T3.init(8);
        run({keys.size()}, one, s1, T1);
        run({333, 950, keys.size()}, three, s3, T3);
        CHECK(one == three);
        for (uint32_t k = 0; k < DD_SCALARS; ++k) CHECK(s1[k] == s3[k]);
        CHECK(s1[DD_READS_SEEN] == keys.size() && s1[DD_ELIGIBLE] == 720 + 300 && s1[DD_ELIGIBLE] - s1[DD_DUPLICATES] == s1[DD_FRAGMENTS] && s1[DD_FRAGMENTS] == T1.entries);
        std::map<uint64_t, size_t> first;
        for (size_t i = 0; i < keys.size(); ++i) {
            const bool dup = keys[i] && first.count(keys[i]);
            if (keys[i] && !dup) first[keys[i]] = i;
            CHECK(one[i] == (dup ? 1 : 0));
        }
        uint64_t hist[kBins] = {};
        T3.histogram(hist);
        CHECK(hist[kBins - 1] == 1 && T3.grows == 2 && T1.grows == 0);  // 8 -> 1024 for 333 reads, -> 2048 for 617 more
    }
    std::printf("dedup selftest ok\n");
    return 0;
}
