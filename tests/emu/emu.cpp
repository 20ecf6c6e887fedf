// emu.cpp — TEST-ONLY host build of the per-read device logic (search_core.hpp / darray_core.hpp).
//
// The kernels' control flow is ordinary C++ on quad-uniform values; only the rank queries are lane-cooperative.  Compiling
// the same headers with g++ (scalar rank queries on the identical block layout) lets the CPU test-suite (-m "not gpu")
// check heap / slab / hit-list / D-array logic, the block layout and the score tables against the oracle without a GPU.
// This library is never loaded by the product (mapad_amd/): it is built into tests/emu/_build by tests/emu_util.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>

#define MAPAD_PC_STATS 1
// Every arena and index access of the host build of the step goes through this hook (csrc/common.hpp: MAPAD_TOUCH): a line-granular model of what lies between a
// read slot and HBM (emu_touch below) attributes the requests of a pop to the structures that cause them.  Off (one predictable branch) unless a caller asks.
extern "C" void emu_touch(const void* p, unsigned long bytes, bool wr);
#define MAPAD_TOUCH(p, bytes, wr) emu_touch((const void*)(p), (unsigned long)(bytes), (wr))
#define MAPAD_PAR_COMMIT_EMU 1  // the lane-parallel commit of the quad kernel, emulated lane by lane (search_core.hpp); runs when the payload cache is off

#include "../../include/mapad_amd.h"
#include "../../mapad_amd/csrc/darray_core.hpp"
#include "../../mapad_amd/csrc/host_models.hpp"
#include "../../mapad_amd/csrc/search_core.hpp"

using namespace mapad;

// ---- request attribution: which lines are the ~5 requests per pop that leave the L2? ------------------------------------------------------------------------
// A read slot's share of the L2 is tiny — 4 MB per XCD over 5 632 resident read slots = 6 lines of 128 B — so each read's traffic is modelled by a private
// fully-associative LRU of `cap` lines (write-back, write-allocate without fetch: the L2 keeps byte masks), for several (line size, capacity) pairs at once.
// Round 6 (the round-5 verdict measured what round 5's model left out): INDEX lines go through the same LRU as the arena's — in the real L2 they evict arena
// lines every pop —, the two rank queries of a pop that fall into one line count once (`index_distinct`: a touch whose line differs from the previous index
// touch's), and write-backs are counted as the memory side counts them: one request per dirty 64-byte half of a line (TCC_EA0_WRREQ: 32- and 64-byte requests).
// The capacity is the calibration knob: profiles/request_attribution.py sweeps it against the PMC figures of C2 and C3 (reads and writes per pop behind the L2).
// The arena's heap levels are seen where the build puts them (heap_core.hpp: HeapLayout — subtree blocks by default, -DMAPAD_SUBTREE_HEAP=0 the implicit array).
namespace {
enum { K_INDEX = 0, K_HEAP = 1, K_NODE = 2, K_HITS = 3, K_OTHER = 4, K_N = 5 };
struct LineCache {
    uint32_t line_shift = 7, cap = 6;
    bool random_victim = false;  // evict a random line instead of the least recently used one: a read's lines sit in a 16-way set-associative L2 among the lines of 5 600 other
                                 // reads, and how long one survives is spread widely (a just-written node line is often gone before its neighbour node is written), not LRU-sharp
    uint32_t clean_after = 0;    // > 0: a dirty line is written back (and stays, clean) once this many other lines have been touched after it — the L2 does not sit on dirty
                                 // data as long as it keeps clean lines (measured: more write requests per pop than any pure write-back LRU of the fitting capacity gives)
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    struct Line { uint64_t addr; uint32_t kind, dirty; };  // dirty: one bit per 64-byte half
    std::vector<Line> lines;  // most recently used last
    uint64_t read_miss[K_N] = {}, writeback[K_N] = {}, access[K_N] = {};
    void evict_front() {
        size_t v = 0;
        if (random_victim) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; v = (size_t)(rng % lines.size()); }
        const Line f = lines[v];
        writeback[f.kind] += (uint64_t)__builtin_popcount(f.dirty);
        lines.erase(lines.begin() + (long)v);
    }
    void touch(uint64_t addr, uint32_t bytes, bool wr, int kind) {
        for (uint64_t ln = addr >> line_shift; ln <= (addr + bytes - 1) >> line_shift; ++ln) {
            access[kind] += 1;
            uint32_t halves = 0;  // 64-byte halves of this line the access covers
            if (wr) {
                const uint64_t lo = std::max<uint64_t>(addr, ln << line_shift), hi = std::min<uint64_t>(addr + bytes, (ln + 1) << line_shift);
                for (uint64_t h = (lo - (ln << line_shift)) >> 6; h <= (hi - 1 - (ln << line_shift)) >> 6; ++h) halves |= 1u << h;
            }
            size_t i = 0;
            for (; i < lines.size(); ++i) if (lines[i].addr == ln) break;
            if (i < lines.size()) {
                Line e = lines[i];
                e.dirty |= halves;
                lines.erase(lines.begin() + (long)i);
                lines.push_back(e);
            } else {
                if (!wr) read_miss[kind] += 1;
                if (lines.size() >= cap) evict_front();
                lines.push_back(Line{ln, (uint32_t)kind, halves});
            }
            if (clean_after && lines.size() > clean_after) {  // the line that has just fallen behind the `clean_after` most recent ones
                Line& o = lines[lines.size() - 1 - clean_after];
                if (o.dirty) { writeback[o.kind] += (uint64_t)__builtin_popcount(o.dirty); o.dirty = 0; }
            }
        }
    }
    void flush() { while (!lines.empty()) { const bool r = random_victim; random_victim = false; evict_front(); random_victim = r; } }
};
struct Attribution {
    bool on = false;
    uint64_t heap_lo = 0, heap_hi = 0, node_lo = 0, node_hi = 0, hits_lo = 0, hits_hi = 0, ops_lo = 0, ops_hi = 0, index_lo = 0, index_hi = 0, near_lo = 0, near_hi = 0;
    std::vector<LineCache> caches;
    uint64_t index_touches = 0, index_distinct = 0, last_index_line = ~0ull, near_touches = 0, pops = 0;
    uint64_t heap_level_reads[32] = {};  // arena heap reads by heap level: where a sift's trips go
} g_attr;
// heap level of a physical entry of the arena's heap area (offset from A.heap): the inverse of HeapLayout<kTop>::slot
int level_of_heap_offset(uint64_t off) {
#if MAPAD_SUBTREE_HEAP
    if (off < (uint64_t)kTop) return 63 - __builtin_clzll(off + 1);
    const uint64_t block = (off - kTop) / 8, s = (off - kTop) % 8;
    int lk = HeapLayout<kTop>::kK0;
    for (uint64_t first = 0; block >= first + (1ull << lk); first += 1ull << lk, lk += 2) {}
    return s < 2 ? lk + 1 : lk + 2;
#else
    return 63 - __builtin_clzll(off + 1);
#endif
}
}  // namespace
extern "C" void emu_touch(const void* p, unsigned long bytes, bool wr) {
    if (!g_attr.on) return;
    uint64_t a = (uint64_t)p;
    int kind = K_OTHER;
    if (a >= g_attr.near_lo && a < g_attr.near_hi) { g_attr.near_touches += 1; return; }  // LDS on the device
    // Addresses are moved to where the DEVICE has the structure: its allocations are aligned to 128 bytes and more (index blocks, an arena's heap area and its
    // node slab), the host's vectors to 16 — a 64-byte index block or a 32-byte node would straddle two lines here that it never straddles there (round 6: the host
    // copy of the 48 Mbp index sat at ...010 and every second block counted as two lines).
    if (a >= g_attr.index_lo && a < g_attr.index_hi) {
        kind = K_INDEX;
        a = (1ull << 44) + (a - g_attr.index_lo);
        g_attr.index_touches += 1;
        if ((a >> 7) != g_attr.last_index_line) g_attr.index_distinct += 1;
        g_attr.last_index_line = a >> 7;
    } else if (a >= g_attr.heap_lo && a < g_attr.heap_hi) {
        kind = K_HEAP;
        if (!wr) g_attr.heap_level_reads[level_of_heap_offset((a - g_attr.heap_lo) / sizeof(HeapEntry)) & 31] += 1;
        a = (2ull << 44) + sizeof(HeapEntry) + (a - g_attr.heap_lo);  // (A.heap points one entry into the aligned allocation)
    }
    else if (a >= g_attr.node_lo && a < g_attr.node_hi) { kind = K_NODE; a = (3ull << 44) + (a - g_attr.node_lo); }
    else if (a >= g_attr.hits_lo && a < g_attr.hits_hi) { kind = K_HITS; a = (4ull << 44) + (a - g_attr.hits_lo); }
    else if (a >= g_attr.ops_lo && a < g_attr.ops_hi) { kind = K_HITS; a = (5ull << 44) + (a - g_attr.ops_lo); }
    for (auto& c : g_attr.caches) c.touch(a, (uint32_t)bytes, wr, kind);
}

namespace {
struct EmuResult {
    mapad_batch_result_t pub{};
    std::vector<uint64_t> hit_begin;
    std::vector<mapad_hit_t> hits;
    std::vector<uint32_t> ops, status;
    std::vector<mapad_read_counters_t> counters;
    std::vector<float> d_arrays;
};
}  // namespace

extern "C" {

// node_cap / heap_cap: arena capacity of the first pass; reads that overflow are re-run with the reference limits.
mapad_batch_result_t* emu_map_batch(const uint64_t* blocks, uint64_t n_blocks, uint64_t n, const uint64_t* less8, const uint64_t* sentinel2,
                                    const mapad_params_t* p, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n_reads,
                                    uint32_t node_cap, uint32_t heap_cap) {
    DevIndex ix;
    ix.blocks = blocks; ix.n = n; ix.n_blocks = n_blocks;
    for (int i = 0; i < 8; ++i) ix.less[i] = less8[i];
    ix.sentinel[0] = sentinel2[0]; ix.sentinel[1] = sentinel2[1];
    host::HostTables t = host::make_tables(*p);
    uint32_t lmax = 1;
    for (uint64_t i = 0; i < n_reads; ++i) { const uint32_t l = (uint32_t)(offsets[i + 1] - offsets[i]); lmax = std::max(lmax, l); if (l) host::add_length(*p, t, (int)l); }
    DevParams P{};
    P.sdm_table = t.sdm.data(); P.table_base = t.table_base.data(); P.reject_thr = t.reject_thr.data();
    P.nq = t.nq; P.bound_kind = p->bound_kind; P.cutoff = p->cutoff; P.repr_mm = t.repr_mm;
    P.gap_open = p->penalty_gap_open; P.gap_extend = p->penalty_gap_extend; P.gap_dist_ends = p->gap_dist_ends; P.max_num_gaps_open = p->max_num_gaps_open;
    P.start_at_end = p->model_kind == MAPAD_MODEL_SIMPLE_ADNA; P.stack_limit_abort = p->stack_limit_abort;
    P.stack_limit = p->stack_limit ? p->stack_limit : 2000000u; P.edit_tree_limit = p->edit_tree_limit ? p->edit_tree_limit : 10000000u;

    auto* r = new EmuResult();
    r->hit_begin.assign(n_reads + 1, 0); r->status.resize(n_reads); r->counters.resize(n_reads);
    r->d_arrays.resize(n_reads ? offsets[n_reads] : 0);
    std::vector<HeapEntry> top(kTop + 1 + 8);  // logical slots [0, kTop) shifted by one, plus slack for pair loads
    // the payload cache of heap slots 1 and 2 (search_step<.., PC>), as the quad kernel runs it; MAPAD_EMU_PAYLOAD_CACHE=0: the plain step
    const char* pc_env = std::getenv("MAPAD_EMU_PAYLOAD_CACHE");
    const bool use_pc = !(pc_env && pc_env[0] == '0');
    uint64_t pc_words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    g_pc_stats[0] = g_pc_stats[1] = g_pc_stats[2] = g_pc_stats[3] = g_pc_stats[4] = 0;
    for (auto& x : g_commit_stats) x = 0;
    for (auto& x : g_par_stats) x = 0;
    std::vector<uint8_t> qc(2 * (lmax + 1));
    std::vector<float> dnear(lmax + 1);
    std::vector<float> pen(lmax + 1), chain;  // (chain: sized per read below)
    std::vector<HeapEntry> heap;
    std::vector<Node> nodes;
    std::vector<HitRec> hits(kMaxHits);
    std::vector<uint32_t> hit_ops(kMaxHits * (lmax + 32));
    std::vector<uint16_t> scratch(2 * (lmax + 2));
    uint64_t second = 0, migrations = 0;
    // host stand-in for DeviceGrow (mapad_amd.hip): up to two x4 migrations of heap slots [kTop, heap_len) and nodes [0, tree_entries)
    std::vector<HeapEntry> gheap[2];
    std::vector<Node> gnodes[2];
    struct HostGrow {
        std::vector<HeapEntry>* gheap; std::vector<Node>* gnodes; uint64_t* migrations; uint32_t stack_cap, tree_cap;
        int operator()(Arena& A, const SearchState& st) const {
            const uint32_t cls = A.grown >> 27;
            if (cls >= 2) return GROW_NEVER;
            const uint32_t hc = std::min<uint64_t>((uint64_t)A.heap_cap * 4, stack_cap), nc = std::min<uint64_t>((uint64_t)A.node_cap * 4, tree_cap);
            gheap[cls].assign(std::max<size_t>(2 * (size_t)hc, HeapLayout<kTop>::phys_end(hc)) + 64, HeapEntry{});
            gnodes[cls].assign(nc, Node{});
            HeapEntry* nheap = gheap[cls].data() + 1;
            for (uint32_t q = kTop + 1; q < HeapLayout<kTop>::phys_end(st.heap_len); ++q) nheap[q - 1] = A.heap[q - 1];  // physical entries, as DeviceGrow copies them
            for (uint32_t i = 0; i < st.tree_entries; ++i) gnodes[cls][i] = A.nodes[i];
            A.heap = nheap; A.nodes = gnodes[cls].data(); A.heap_cap = hc; A.node_cap = nc; A.grown = ((cls + 1) << 27) | 1u;
            ++*migrations;
            return GROW_OK;
        }
    };
    const HostGrow grow{gheap, gnodes, &migrations, P.stack_limit + 10, P.edit_tree_limit + 10};
    for (uint64_t i = 0; i < n_reads; ++i) {
        const uint64_t off = offsets[i];
        const int L = (int)(offsets[i + 1] - off);
        float* d = r->d_arrays.data() + off;
        ReadCounters ctr{};
        {   // (the D arrays are another kernel's work — darray_kernel —: not part of the search step's requests)
            const bool attr_was_on = g_attr.on;
            g_attr.on = false;
            // a chain buffer of exactly this read's length with guard words behind it: d_chain may write out[0 .. part_len) only (on the device the chains of a
            // read lie back to back in 16 x lmax floats, the last one at the end of the allocation).  A trampled guard poisons the read's D array, which the
            // comparison with the oracle then reports — a caller that does not compare D arrays (assert_same_as_oracle without keep_d) sees only the line on stderr.
            constexpr uint32_t kGuard = 0x7FC0DEADu;  // (a NaN no chain computes)
            constexpr int kGuards = 16;  // > kMaxOffset
            chain.assign((size_t)L + kGuards, 0.0f);
            for (int k = 0; k < kGuards; ++k) std::memcpy(&chain[(size_t)L + k], &kGuard, 4);
            ctr.e_darray = d_array_scalar(ix, P, seqs + off, quals + off, L, pen.data(), chain.data(), d);
            for (int k = 0; k < kGuards; ++k) {
                uint32_t v; std::memcpy(&v, &chain[(size_t)L + k], 4);
                if (v != kGuard) {
                    std::fprintf(stderr, "emu: read %llu (%d bases): a D-array chain wrote %d floats past its part\n", (unsigned long long)i, L, k + 1);
                    for (int r = 0; r < L; ++r) std::memcpy(&d[r], &kGuard, 4);
                    break;
                }
            }
            g_attr.on = attr_was_on;
        }
        read_setup(seqs + off, quals + off, d, L, qc.data(), dnear.data(), 0, 1);
        SearchState st;
        for (int pass = 0; pass < 3; ++pass) {
            // pass 1 runs with the reference's limits in backing stores of at most 2^22 entries, which keeps the host emulation cheap (the limits are 2M / 10M); a
            // read whose edit tree outgrows 2^22 nodes below its limit is run once more, pass 2, in stores as large as the limits (10 M nodes and 4 M heap entries
            // with the reference's limits — also for a read that left pass 1 with an arena overflow for another reason, such as its hit_ops area: rare, and only slower)
            const uint32_t store_max = pass == 1 ? 1u << 22 : 0xFFFFFFFFu;
            const uint32_t hc = std::min(pass == 0 ? heap_cap : P.stack_limit + 10, store_max), nc = std::min(pass == 0 ? node_cap : P.edit_tree_limit + 10, store_max);
            Arena A;
            heap.assign(std::max<size_t>(2 * (size_t)hc, HeapLayout<kTop>::phys_end(hc)) + 64, HeapEntry{});  // implicit array: a sift reads (and ignores) slots up to 2 * heap_len + 6: twice the capacity, as in host_tail.hpp
            nodes.assign(nc, Node{});
            A.top = top.data() + 1; A.heap = heap.data() + 1; A.nodes = nodes.data(); A.hits = hits.data(); A.hit_ops = hit_ops.data(); A.scratch = scratch.data();
            A.heap_cap = hc; A.node_cap = (uint32_t)nodes.size(); A.hit_ops_cap = (uint32_t)hit_ops.size();
            A.pc = use_pc ? pc_words : nullptr;
            ReadIn rd{qc.data(), dnear.data(), L, P.reject_thr[L], P.table_base[L]};
            if (g_attr.on) {  // (the attribution run gives every read an arena it cannot outgrow: no migrations, one set of address ranges per read)
                g_attr.heap_lo = (uint64_t)A.heap; g_attr.heap_hi = (uint64_t)(heap.data() + heap.size());
                g_attr.node_lo = (uint64_t)nodes.data(); g_attr.node_hi = (uint64_t)(nodes.data() + nodes.size());
                g_attr.hits_lo = (uint64_t)hits.data(); g_attr.hits_hi = (uint64_t)(hits.data() + hits.size());
                g_attr.ops_lo = (uint64_t)hit_ops.data(); g_attr.ops_hi = (uint64_t)(hit_ops.data() + hit_ops.size());
                g_attr.near_lo = (uint64_t)top.data(); g_attr.near_hi = (uint64_t)(top.data() + top.size());
                g_attr.index_lo = (uint64_t)ix.blocks; g_attr.index_hi = (uint64_t)(ix.blocks + ix.n_blocks * mapad::kBlockWords);
            }
            if (pass == 0) search_read(ix, P, rd, A, st, 0, grow);
            else search_read(ix, P, rd, A, st, 0);
            if (st.status != ST_ARENA_OVERFLOW) break;
            if (pass == 0) second += 1;
            if (pass == 1 && hc >= P.stack_limit + 10 && nc >= P.edit_tree_limit + 10) break;  // (the stores were as large as the limits already)
        }
        if (g_attr.on) { for (auto& c : g_attr.caches) c.flush(); g_attr.pops += st.c_pop; }
        r->status[i] = st.status;
        ctr.e_search = st.c_esearch; ctr.n_push = st.c_push; ctr.n_pop = st.c_pop; ctr.n_node = st.c_node; ctr.n_hits = st.c_hits;
        std::memcpy(&r->counters[i], &ctr, sizeof ctr);
        for (uint32_t k = 0; k < st.n_hits; ++k) {
            const HitRec& h = hits[k];
            mapad_hit_t o{h.lower, h.lower_rev, h.size, h.score, h.n_ops, (uint32_t)r->ops.size(), 0};
            r->ops.insert(r->ops.end(), hit_ops.begin() + h.ops_off, hit_ops.begin() + h.ops_off + h.n_ops);
            r->hits.push_back(o);
        }
        r->hit_begin[i + 1] = r->hits.size();
    }
    if (std::getenv("MAPAD_EMU_PC_STATS")) std::fprintf(stderr, "emu commit loop: %llu steps with children, %llu children, %llu movers, %llu steps without a mover; >= 3 children: %llu steps, %llu without a mover, %llu movers\n",
                                                       g_commit_stats[0], g_commit_stats[1], g_commit_stats[2], g_commit_stats[3], g_commit_stats[4], g_commit_stats[5], g_commit_stats[6]);
    if (std::getenv("MAPAD_EMU_PC_STATS")) std::fprintf(stderr, "emu lane-parallel commit: %llu rounds with >= 2 movers, %llu movers in them = rounds of bubble-ups one after the other; %llu rounds with the parallel prefix\n", g_par_stats[0], g_par_stats[1], g_par_stats[2]);
    if (std::getenv("MAPAD_EMU_PC_STATS")) std::fprintf(stderr, "emu payload cache: %llu hits, %llu misses, %llu pops of a one-entry heap; %llu nodes fetched ahead, %llu steps with a child landing in slot 1 / 2\n", g_pc_stats[0], g_pc_stats[1], g_pc_stats[2], g_pc_stats[3], g_pc_stats[4]);
    r->pub.n_reads = n_reads; r->pub.n_hits = r->hits.size(); r->pub.n_ops = r->ops.size();
    r->pub.hit_begin = r->hit_begin.data(); r->pub.hits = r->hits.data(); r->pub.ops = r->ops.data(); r->pub.status = r->status.data();
    r->pub.counters = r->counters.data(); r->pub.d_arrays = r->d_arrays.data(); r->pub.n_second_pass = migrations; r->pub.n_third_pass = second;
    return &r->pub;
}
void emu_result_free(mapad_batch_result_t* r) { if (r) delete reinterpret_cast<EmuResult*>(r); }

// Request attribution: emu_attr_begin(configs as (line_shift, capacity) pairs) ... emu_map_batch(...) ... emu_attr_end(out): per config and structure
// {accesses, read misses, write-backs}, then the totals.  out: n_cfg x 5 kinds x 3 u64, then {pops, index touches, near touches, distinct index lines}, then 32 heap-level read counts.
void emu_attr_begin(const uint32_t* cfg, uint32_t n_cfg) {
    g_attr = Attribution();
    for (uint32_t i = 0; i < n_cfg; ++i) { LineCache c; c.line_shift = cfg[2 * i] & 0xFF; c.random_victim = (cfg[2 * i] >> 8) & 1; c.clean_after = cfg[2 * i] >> 16; c.cap = cfg[2 * i + 1]; g_attr.caches.push_back(c); }  // (line shift | random replacement << 8 | clean-after << 16, capacity)
    g_attr.on = true;
}
void emu_attr_end(uint64_t* out) {
    g_attr.on = false;
    size_t k = 0;
    for (auto& c : g_attr.caches) for (int kind = 0; kind < K_N; ++kind) { out[k++] = c.access[kind]; out[k++] = c.read_miss[kind]; out[k++] = c.writeback[kind]; }
    out[k++] = g_attr.pops; out[k++] = g_attr.index_touches; out[k++] = g_attr.near_touches; out[k++] = g_attr.index_distinct;
    for (int l = 0; l < 32; ++l) out[k++] = g_attr.heap_level_reads[l];
}

// Property check of fmd_device.hpp's row -> (block, row in block) split (a division by 96 written as 32-bit arithmetic): `trials` random rows below 2^bits plus
// the rows around every power of two and around multiples of 96 * 65536.  Returns the number of rows it gets wrong (must be 0).
uint64_t emu_block_pos_selftest(uint64_t seed, uint32_t trials, uint32_t bits) {
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1, bad = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    auto check = [&](uint64_t r) {
        if (r >> bits) return;
        const BlockPos p = block_pos(r);
        bad += (p.b != r / (uint64_t)kBlockRows) || (p.r_in != (int)(r % (uint64_t)kBlockRows));
    };
    for (uint32_t t = 0; t < trials; ++t) check(rnd() >> (64 - bits));
    for (uint32_t k = 0; k < bits; ++k) for (int64_t d = -200; d <= 200; ++d) if ((int64_t)(1ull << k) + d >= 0) check((1ull << k) + (uint64_t)d);
    for (uint64_t m = 0; m < 4096; ++m) for (int64_t d = -3; d <= 3; ++d) if (m || d >= 0) check(m * 96u * 65536u + (uint64_t)d);
    return bad;
}

// Property check of the lane-parallel commit (search_core.hpp: MAPAD_PAR_COMMIT) on random heaps: `trials` times a min-max heap of n0 in [16, max_n] entries is
// built by sequential pushes of scores drawn from `levels` distinct values (few levels = many ties, the common case of the no-damage model), then k in [1, 9]
// children are pushed (a) one after the other (the reference's order) and (b) by the scheme — four at a time: every child decides against the heap as it stands
// whether it stays (mm_push_stays), the stayers are stored, the movers follow in commit order with freshly loaded ancestors.  Returns the number of trials in
// which the two heaps differ in any slot (must be 0).
uint64_t emu_par_commit_selftest(uint64_t seed, uint32_t trials, uint32_t max_n, uint32_t levels) {
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1, bad = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    std::vector<HeapEntry> top_a(kTop + 9), top_b(kTop + 9), heap_a(2 * (size_t)max_n + 256), heap_b(2 * (size_t)max_n + 256);
    for (uint32_t t = 0; t < trials; ++t) {
        Arena A, B;
        A.top = top_a.data() + 1; A.heap = heap_a.data() + 1; B.top = top_b.data() + 1; B.heap = heap_b.data() + 1;
        const uint32_t n0 = 16 + (uint32_t)(rnd() % (max_n - 15));
        auto score = [&]() { return -(float)(rnd() % levels) * 0.75f; };
        uint32_t n = 0;
        for (uint32_t i = 0; i < n0; ++i) { mm_bubble_up(A, n, HeapEntry{score(), i}); n += 1; }
        for (uint32_t i = 0; i < n0; ++i) hp_set(B, i, hp_get(A, i));
        const uint32_t k = 1 + (uint32_t)(rnd() % 9);
        HeapEntry kid[9];
        for (uint32_t i = 0; i < k; ++i) kid[i] = HeapEntry{score(), n0 + i};
        for (uint32_t i = 0; i < k; ++i) mm_bubble_up(A, n0 + i, kid[i]);                     // (a)
        for (uint32_t base = 0; base < k; base += 4) {                                         // (b)
            Ancestors an[4];
            uint32_t movers = 0;
            for (uint32_t w = 0; w < 4 && base + w < k; ++w) an[w] = load_ancestors(B, n0 + base + w);
            for (uint32_t w = 0; w < 4 && base + w < k; ++w) {
                if (mm_push_stays(n0 + base + w, kid[base + w], an[w])) hp_set(B, n0 + base + w, kid[base + w]); else movers |= 1u << w;
            }
            bool fresh = true;
            for (uint32_t w = 0; w < 4; ++w) if ((movers >> w) & 1u) {
                if (fresh) mm_bubble_up(B, n0 + base + w, kid[base + w], an[w]); else mm_bubble_up(B, n0 + base + w, kid[base + w]);
                fresh = false;
            }
        }
        bool same = true;
        for (uint32_t i = 0; i < n0 + k && same; ++i) { const HeapEntry a = hp_get(A, i), b = hp_get(B, i); same = a.score == b.score && a.node == b.node; }
        bad += same ? 0 : 1;
    }
    return bad;
}

}  // extern "C"
