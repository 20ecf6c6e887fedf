// tail_ring_selftest.cpp — TEST-ONLY stand-alone program for the host half of the host tail (mapad_amd/csrc/host_tail.hpp) without a GPU: tail_start's
// dispatcher, TailWorkers, tail_map_read, tail_finish and tail_cancel are the product's; the kernel's half is played by producer threads that build each record's
// payload as tests/emu/tail_bench.cpp does, claim ring slots by the rule of search_kernel's give_to_host (restated below) and publish `ready = gen` with release
// order.  The ring is ordinary memory and `fetch_state` stays empty: every record is mapped from scratch.  Built and run by tests/test_tail_host.py — plain, under
// ThreadSanitizer and under AddressSanitizer + UBSan —, which writes the input file (index blocks, parameters, reads, the oracle's pops per read).
// Exit status 0 and "tail ring selftest ok" on stdout: every case held.
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <thread>
#include <vector>

#include "../../include/mapad_amd.h"
#include "../../mapad_amd/csrc/darray_core.hpp"
#include "../../mapad_amd/csrc/host_models.hpp"
#include "../../mapad_amd/csrc/host_tail.hpp"

using namespace mapad;

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// ---- the input --------------------------------------------------------------------------------------------------------------------------------------------------
struct Input {
    std::vector<uint64_t> blocks, offsets, want_pops;
    std::vector<uint8_t> seqs, quals;
    mapad_params_t params{};
    DevIndex ix{};
    uint64_t n_reads = 0;
};

static bool load(const char* path, Input& in) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint64_t h[16];  // magic, n_blocks, n, less[8], sentinel[2], sizeof(mapad_params_t), n_reads, total bases
    bool ok = std::fread(h, 8, 16, f) == 16 && h[0] == 0x4C49415444415041ull && h[13] == sizeof(mapad_params_t);
    if (ok) {
        in.ix.n_blocks = h[1]; in.ix.n = h[2];
        for (int i = 0; i < 8; ++i) in.ix.less[i] = h[3 + i];
        in.ix.sentinel[0] = h[11]; in.ix.sentinel[1] = h[12];
        in.n_reads = h[14];
        in.blocks.resize(h[1] * kBlockWords); in.offsets.resize(h[14] + 1); in.want_pops.resize(h[14]); in.seqs.resize(h[15]); in.quals.resize(h[15]);
        ok = std::fread(in.blocks.data(), 8, in.blocks.size(), f) == in.blocks.size() && std::fread(&in.params, sizeof in.params, 1, f) == 1 &&
             std::fread(in.offsets.data(), 8, in.offsets.size(), f) == in.offsets.size() && std::fread(in.seqs.data(), 1, in.seqs.size(), f) == in.seqs.size() &&
             std::fread(in.quals.data(), 1, in.quals.size(), f) == in.quals.size() && std::fread(in.want_pops.data(), 8, in.want_pops.size(), f) == in.want_pops.size();
        in.ix.blocks = in.blocks.data();
    }
    std::fclose(f);
    return ok;
}

// ---- what every case shares: tables, the payload of every read's record, and the result of mapping the read directly (tail_bench.cpp's loop body) ---------------
struct World {
    Input in;
    std::shared_ptr<const host::HostTables> tables;
    DevParams P{};
    uint32_t lmax = 1, stride = 0;
    std::vector<std::vector<uint8_t>> qc;   // per read: ReadIn::qc as read_setup lays it out
    std::vector<std::vector<float>> dnear;  // per read: the D array as read_setup lays it out
    std::vector<uint64_t> digest, pops;     // per read: of the direct tail_search
    std::vector<uint32_t> by_weight;        // read numbers, heaviest first
};

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void mix(uint64_t v) { h = (h ^ v) * 1099511628211ull; }
};
// the digest of tests/emu/tail_bench.cpp: status, the five counters, the hits (interval, score bits, track length), the edit tracks
static uint64_t digest_of(uint32_t status, uint32_t e_search, uint32_t n_push, uint32_t n_pop, uint32_t n_node, uint32_t c_hits, const HitRec* hits, uint32_t n_hits,
                          const uint32_t* ops, uint32_t n_ops) {
    Fnv f;
    f.mix(status); f.mix(e_search); f.mix(n_push); f.mix(n_pop); f.mix(n_node); f.mix(c_hits); f.mix(n_hits);
    for (uint32_t q = 0; q < n_hits; ++q) { const HitRec& hr = hits[q]; f.mix(hr.lower); f.mix(hr.lower_rev); f.mix(hr.size); uint32_t sb; std::memcpy(&sb, &hr.score, 4); f.mix(sb); f.mix(hr.n_ops); }
    for (uint32_t q = 0; q < n_ops; ++q) f.mix(ops[q]);
    return f.h;
}

static void prepare(World& w) {
    const Input& in = w.in;
    const mapad_params_t* p = &in.params;
    host::HostTables t = host::make_tables(*p);
    for (uint64_t i = 0; i < in.n_reads; ++i) { const uint32_t l = (uint32_t)(in.offsets[i + 1] - in.offsets[i]); w.lmax = std::max(w.lmax, l); if (l) host::add_length(*p, t, (int)l); }
    w.tables = std::make_shared<const host::HostTables>(std::move(t));
    DevParams& P = w.P;
    P.sdm_table = w.tables->sdm.data(); P.table_base = w.tables->table_base.data(); P.reject_thr = w.tables->reject_thr.data();
    P.nq = w.tables->nq; P.bound_kind = p->bound_kind; P.cutoff = p->cutoff; P.repr_mm = w.tables->repr_mm;
    P.gap_open = p->penalty_gap_open; P.gap_extend = p->penalty_gap_extend; P.gap_dist_ends = p->gap_dist_ends; P.max_num_gaps_open = p->max_num_gaps_open;
    P.start_at_end = p->model_kind == MAPAD_MODEL_SIMPLE_ADNA; P.stack_limit_abort = p->stack_limit_abort;
    P.stack_limit = p->stack_limit; P.edit_tree_limit = p->edit_tree_limit;  // (small, set by the test: a worker's arena is megabytes)
    w.stride = host::tail_record_stride(w.lmax);
    const uint32_t lmax = w.lmax;
    w.qc.resize(in.n_reads); w.dnear.resize(in.n_reads); w.digest.resize(in.n_reads); w.pops.resize(in.n_reads);
    std::vector<float> d(lmax + 1), pen(lmax + 1), chain(lmax + 1);
    host::TailScratch sc;
    for (uint64_t i = 0; i < in.n_reads; ++i) {
        const uint64_t off = in.offsets[i];
        const int L = (int)(in.offsets[i + 1] - off);
        w.qc[i].assign(2 * (lmax + 1), 0); w.dnear[i].assign(lmax + 1, 0.0f);
        d_array_scalar(in.ix, P, in.seqs.data() + off, in.quals.data() + off, L, pen.data(), chain.data(), d.data());
        read_setup(in.seqs.data() + off, in.quals.data() + off, d.data(), L, w.qc[i].data(), w.dnear[i].data(), 0, 1);
        if (!sc.ensure(P.stack_limit + 10, P.edit_tree_limit + 10, lmax)) { CHECK(false, "no arena"); return; }
        Arena A;
        A.top = sc.top.data() + 1; A.heap = sc.heap + 1; A.nodes = sc.nodes; A.hits = sc.hits.data(); A.hit_ops = sc.hit_ops.data(); A.scratch = sc.scratch.data();
        A.heap_cap = sc.heap_cap; A.node_cap = sc.node_cap; A.hit_ops_cap = (uint32_t)sc.hit_ops.size();
        A.pc = sc.pc;
        const ReadIn rd{w.qc[i].data(), w.dnear[i].data(), L, P.reject_thr[L], P.table_base[L]};
        SearchState st;
        host::tail_search(in.ix, P, rd, A, st, 0, nullptr);
        w.pops[i] = st.c_pop;
        w.digest[i] = digest_of(st.status, st.c_esearch, st.c_push, st.c_pop, st.c_node, st.c_hits, sc.hits.data(), st.n_hits, sc.hit_ops.data(), st.hit_ops_used);
        CHECK(st.c_pop == in.want_pops[i], "read %llu: %u pops, the oracle made %llu", (unsigned long long)i, st.c_pop, (unsigned long long)in.want_pops[i]);
    }
    w.by_weight.resize(in.n_reads);
    for (uint32_t i = 0; i < in.n_reads; ++i) w.by_weight[i] = i;
    std::stable_sort(w.by_weight.begin(), w.by_weight.end(), [&](uint32_t a, uint32_t b) { return w.pops[a] > w.pops[b]; });
}

// ---- the kernel's half --------------------------------------------------------------------------------------------------------------------------------------------
// A slot's ring as launch_batch sets it up (mapad_amd.hip: launch_batch, "ctl[0] = ...pending(); ctl[1] = 0"): two control words, the records, and the launch's
// ring cursor (cursors[CUR_TAIL] on the device).
struct Ring {
    std::unique_ptr<uint8_t[]> mem;
    uint32_t ctl[2] = {0, 0};
    uint32_t stride = 0, holds = 0, gen = 0;
    std::atomic<uint32_t> cursor{0};
    Ring(uint32_t stride_, uint32_t holds_) : mem(new uint8_t[(size_t)stride_ * holds_]()), stride(stride_), holds(holds_) {}  // zeroed: no `ready` word holds a launch number
};

struct Launch {
    std::shared_ptr<host::TailBatch> tb;
    Ring* ring = nullptr;
    uint32_t cap = 0, serial0 = 0;
    std::vector<uint32_t> read_of;  // per record serial (TailRecord::read - serial0): the read it carries
};

static uint32_t g_serial = 0;  // TailRecord::read of this program's records: a number no other launch of the run uses, so a stale record cannot pass for a new one

// launch_batch's part (mapad_amd.hip: "auto tb = std::make_shared<host::TailBatch>()" ... "host::tail_start(tb)")
static Launch start_launch(const World& w, Ring& ring, uint32_t cap) {
    Launch l;
    l.ring = &ring; l.cap = cap; l.serial0 = g_serial;
    g_serial += 1u << 20;
    ring.cursor.store(0);
    ring.gen += 1;
    __atomic_store_n(&ring.ctl[0], host::TailWorkers::instance().pending(), __ATOMIC_RELAXED);
    __atomic_store_n(&ring.ctl[1], 0u, __ATOMIC_RELAXED);
    auto tb = std::make_shared<host::TailBatch>();
    tb->ix = w.in.ix; tb->tables = w.tables; tb->P = w.P;
    tb->ring = ring.mem.get(); tb->stride = ring.stride; tb->cap = cap; tb->lmax = w.lmax; tb->ctl = ring.ctl; tb->gen = ring.gen;
    tb->fetched.assign(cap, 0);
    host::tail_start(tb);
    l.tb = tb;
    return l;
}

// search_kernel's give_to_host (mapad_amd.hip lines 1788-1808), lane 0's part in plain C++: 0 = slot k is the caller's, 1 = refused (backlog), 2 = the ring is full.
//   limit == 0xFFFFFFFF: `k = atomicAdd(&cursors[CUR_TAIL], 1u)` (line 1793)
//   otherwise: the two host words, then the cursor, and a CAS under `pend + (cur - seen) < limit` (lines 1795-1804)
// After a claim under a limit the claimer checks the limit against the TRUE pick-up count (the dispatcher's word as it is now): the kernel's view of it can only lag,
// so the records claimed and not yet picked up never exceed the limit.
static std::atomic<uint32_t> g_max_unpicked{0};
static int claim(Ring& r, uint32_t cap, uint32_t limit, uint32_t& k_out) {
    if (cap == 0) return 2;
    uint32_t k = 0xFFFFFFFEu;
    if (limit == 0xFFFFFFFFu) k = r.cursor.fetch_add(1u, std::memory_order_relaxed);
    else {
        const uint32_t seen = __atomic_load_n(&r.ctl[1], __ATOMIC_RELAXED);
        const uint32_t pend = __atomic_load_n(&r.ctl[0], __ATOMIC_RELAXED);
        uint32_t cur = r.cursor.load(std::memory_order_relaxed);
        for (;;) {
            if (cur >= cap) { k = 0xFFFFFFFFu; break; }
            if ((uint64_t)pend + (cur > seen ? cur - seen : 0u) >= limit) break;
            if (r.cursor.compare_exchange_strong(cur, cur + 1u, std::memory_order_relaxed)) { k = cur; break; }
        }
        if (k < cap) {
            const uint32_t picked = __atomic_load_n(&r.ctl[1], __ATOMIC_ACQUIRE);
            const uint32_t unpicked = k + 1u > picked ? k + 1u - picked : 0u;
            uint32_t m = g_max_unpicked.load(std::memory_order_relaxed);
            while (unpicked > m && !g_max_unpicked.compare_exchange_weak(m, unpicked, std::memory_order_relaxed)) {}
        }
    }
    if (k >= cap) return k == 0xFFFFFFFEu ? 1 : 2;
    k_out = k;
    return 0;
}

// hand_to_host (mapad_amd.hip lines 1566-1601): payload, header, "no state", then the word the host polls
static void publish(const World& w, const Launch& l, uint32_t k, uint32_t serial, uint32_t read, uint32_t pops) {
    uint8_t* rec = l.ring->mem.get() + (size_t)k * l.ring->stride;
    const uint32_t L = (uint32_t)(w.in.offsets[read + 1] - w.in.offsets[read]);
    std::memcpy(rec + 16, w.qc[read].data(), 4u * ((2u * L + 3u) / 4u));
    std::memcpy(rec + 16 + ((2u * w.lmax + 15u) & ~15u), w.dnear[read].data(), 4u * L);
    host::TailRecord* h = reinterpret_cast<host::TailRecord*>(rec);
    h->read = serial; h->L = L; h->pops = pops;
    std::memset(rec + host::tail_state_offset(w.lmax), 0, 4);  // TailState::grown = 0
    __atomic_store_n(&h->ready, l.ring->gen, __ATOMIC_RELEASE);
}

struct Produced {
    uint32_t handed = 0, refusals = 0, ring_full = 0, stayed = 0;
};
// `reads[i]` is offered by one of `threads` producers; a refused read "goes on on the GPU" and asks again, up to `max_asks` times (0: until it is taken).
static Produced produce(const World& w, Launch& l, const std::vector<uint32_t>& reads, uint32_t limit, unsigned threads, uint32_t max_asks) {
    l.read_of.assign(reads.size(), 0);
    for (size_t i = 0; i < reads.size(); ++i) l.read_of[i] = reads[i];
    std::atomic<uint32_t> next{0}, handed{0}, refusals{0}, full{0}, stayed{0};
    std::vector<std::thread> th;
    for (unsigned t = 0; t < threads; ++t) th.emplace_back([&] {
        for (;;) {
            const uint32_t i = next.fetch_add(1);
            if (i >= reads.size()) break;
            uint32_t k = 0, asks = 0;
            int rc;
            while ((rc = claim(*l.ring, l.cap, limit, k)) == 1) {
                refusals.fetch_add(1);
                if (max_asks && ++asks >= max_asks) break;
                std::this_thread::sleep_for(std::chrono::microseconds(50));
            }
            if (rc == 0) { publish(w, l, k, l.serial0 + i, reads[i], 100 + i % 7); handed.fetch_add(1); }
            else if (rc == 2) full.fetch_add(1);
            else stayed.fetch_add(1);
        }
    });
    for (auto& x : th) x.join();
    Produced p;
    p.handed = handed; p.refusals = refusals; p.ring_full = full; p.stayed = stayed;
    return p;
}

// every result of the launch is the direct search's of the read its record carried, and every record handed over has exactly one result
static void check_results(const World& w, const Launch& l, uint32_t handed, const char* what) {
    std::lock_guard<std::mutex> g(l.tb->mu);
    CHECK(l.tb->done == l.tb->dispatched && l.tb->dispatched == handed, "%s: done %u dispatched %u handed over %u", what, l.tb->done, l.tb->dispatched, handed);
    CHECK(l.tb->results.size() == handed && !l.tb->failed, "%s: %zu results", what, l.tb->results.size());
    std::set<uint32_t> seen;
    uint64_t host_pops = 0;
    for (const host::TailResult& r : l.tb->results) {
        const uint32_t i = r.read - l.serial0;
        if (r.read < l.serial0 || i >= l.read_of.size()) { CHECK(false, "%s: a result for record %u, which is not of this launch (%u ..)", what, r.read, l.serial0); continue; }
        CHECK(seen.insert(i).second, "%s: record %u mapped twice", what, i);
        const uint32_t read = l.read_of[i];
        const uint64_t d = digest_of(r.status, r.e_search, r.n_push, r.n_pop, r.n_node, r.n_hits, r.hits.data(), (uint32_t)r.hits.size(), r.ops.data(), (uint32_t)r.ops.size());
        CHECK(d == w.digest[read] && r.n_pop == w.pops[read], "%s: read %u through the ring differs from the direct search (%u pops, %llu)", what, read, r.n_pop, (unsigned long long)w.pops[read]);
        host_pops += r.n_pop;
    }
    CHECK(l.tb->host_pops == host_pops && l.tb->continued == 0, "%s: host_pops %llu, results add up to %llu", what, (unsigned long long)l.tb->host_pops, (unsigned long long)host_pops);
}

static std::vector<uint32_t> cycle(const World& w, uint32_t n, uint32_t from) {
    std::vector<uint32_t> r(n);
    for (uint32_t i = 0; i < n; ++i) r[i] = (from + i) % (uint32_t)w.in.n_reads;
    return r;
}

static bool wait_until(const std::function<bool()>& f, double seconds) {
    const auto t0 = std::chrono::steady_clock::now();
    while (!f()) {
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) return false;
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    return true;
}

// ---- the cases --------------------------------------------------------------------------------------------------------------------------------------------------
static void case_every_record(const World& w) {  // unconditional hand-over (atomicAdd), six producers: every read once
    Ring ring(w.stride, (uint32_t)w.in.n_reads);
    Launch l = start_launch(w, ring, (uint32_t)w.in.n_reads);
    const Produced p = produce(w, l, cycle(w, (uint32_t)w.in.n_reads, 0), 0xFFFFFFFFu, 6, 0);
    CHECK(host::tail_finish(l.tb, ring.cursor.load()), "tail_finish");
    CHECK(p.handed == w.in.n_reads && p.refusals == 0 && p.ring_full == 0, "handed %u", p.handed);
    check_results(w, l, p.handed, "every record");
}

static void case_limit(const World& w, uint32_t limit) {  // CAS under the backlog
    const uint32_t n = 300;
    Ring ring(w.stride, n);
    Launch l = start_launch(w, ring, n);
    g_max_unpicked.store(0);
    const Produced p = produce(w, l, cycle(w, n, 17), limit, 6, limit ? 0 : 3);
    CHECK(host::tail_finish(l.tb, ring.cursor.load()), "tail_finish");
    if (limit == 0) {
        CHECK(p.handed == 0 && p.stayed == n && p.refusals == 3 * n && ring.cursor.load() == 0, "limit 0: %u handed over, %u refusals", p.handed, p.refusals);
        check_results(w, l, 0, "limit 0");
    } else {
        CHECK(p.handed == n && p.stayed == 0 && p.ring_full == 0, "limit %u: %u handed over", limit, p.handed);
        CHECK(g_max_unpicked.load() >= 1 && g_max_unpicked.load() <= limit, "limit %u: %u records claimed and not picked up", limit, g_max_unpicked.load());
        check_results(w, l, n, "limit");
        std::printf("limit %u: %u refusals, at most %u records claimed and not yet picked up\n", limit, p.refusals, g_max_unpicked.load());
    }
}

static void case_generations(const World& w) {  // one ring over five launches (tests/test_gpu_tail.py: the stale-`ready` case, on the host)
    Ring ring(w.stride, 300);
    uint32_t from = 0;
    for (uint32_t n : {300u, 10u, 300u, 10u, 250u}) {
        Launch l = start_launch(w, ring, n);  // (cap = min(reads of the batch, ring): records beyond it keep the `ready` words of earlier launches)
        std::this_thread::sleep_for(std::chrono::milliseconds(3));  // the dispatcher polls records of earlier launches meanwhile: none of them is this launch's
        {
            std::lock_guard<std::mutex> g(l.tb->mu);
            CHECK(l.tb->dispatched == 0, "launch %u of the ring: %u records taken before one was written", ring.gen, l.tb->dispatched);
        }
        const Produced p = produce(w, l, cycle(w, n, from), 0xFFFFFFFFu, 4, 0);
        CHECK(host::tail_finish(l.tb, ring.cursor.load()), "tail_finish");
        CHECK(p.handed == n, "launch %u: %u handed over", ring.gen, p.handed);
        check_results(w, l, n, "generations");
        from += n;
    }
}

static void case_clamp(const World& w) {  // more claims than records (atomicAdd form): the cursor ends beyond the ring, tail_finish clamps
    Ring ring(w.stride, 16);
    Launch l = start_launch(w, ring, 16);
    const Produced p = produce(w, l, cycle(w, 40, 5), 0xFFFFFFFFu, 6, 0);
    CHECK(ring.cursor.load() == 40 && p.handed == 16 && p.ring_full == 24, "cursor %u handed %u", ring.cursor.load(), p.handed);
    CHECK(host::tail_finish(l.tb, ring.cursor.load()), "tail_finish");
    check_results(w, l, 16, "clamp");
}

static void case_cancel(const World& w) {  // tasks queued and running; afterwards the ring (the slot's memory) is gone and nobody may touch it
    const uint32_t n = 2000, heavy = std::max<uint32_t>(1, (uint32_t)w.in.n_reads / 4);
    std::vector<uint32_t> reads(n);
    for (uint32_t i = 0; i < n; ++i) reads[i] = w.by_weight[i % heavy];
    auto ring = std::make_unique<Ring>(w.stride, n);
    Launch l = start_launch(w, *ring, n);
    const Produced p = produce(w, l, reads, 0xFFFFFFFFu, 4, 0);
    CHECK(p.handed == n, "handed %u", p.handed);
    CHECK(wait_until([&] { std::lock_guard<std::mutex> g(l.tb->mu); return l.tb->dispatched >= 50; }, 30.0), "the dispatcher took nothing");
    uint32_t dispatched0, done0;
    { std::lock_guard<std::mutex> g(l.tb->mu); dispatched0 = l.tb->dispatched; done0 = l.tb->done; }
    CHECK(done0 < dispatched0, "nothing queued or running when the batch is cancelled (%u of %u done)", done0, dispatched0);
    host::tail_cancel(l.tb);
    uint32_t dispatched1, done1;
    { std::lock_guard<std::mutex> g(l.tb->mu); dispatched1 = l.tb->dispatched; done1 = l.tb->done; }
    CHECK(done1 == dispatched1 && dispatched1 <= n, "after tail_cancel: done %u dispatched %u", done1, dispatched1);
    std::memset(ring->mem.get(), 0xEE, (size_t)ring->stride * ring->holds);
    ring.reset();  // (under AddressSanitizer a later access is a report)
    CHECK(wait_until([] { return host::TailWorkers::instance().pending() == 0; }, 30.0), "tasks left in the pool");
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    { std::lock_guard<std::mutex> g(l.tb->mu); CHECK(l.tb->done == done1 && l.tb->dispatched == dispatched1 && l.tb->results.size() == done1, "the cancelled batch moved: done %u", l.tb->done); }
    std::printf("cancel: %u of %u records dispatched, %u done at the cancel\n", dispatched1, n, done0);
}

static void case_two_batches(const World& w) {  // one pool per process: the backlog word of each launch counts the tasks of both
    const uint32_t n = 1500, heavy = std::max<uint32_t>(1, (uint32_t)w.in.n_reads / 4);
    std::vector<uint32_t> reads(n);
    for (uint32_t i = 0; i < n; ++i) reads[i] = w.by_weight[i % heavy];
    Ring ra(w.stride, n), rb(w.stride, 200);
    Launch a = start_launch(w, ra, n), b = start_launch(w, rb, 200);
    const Produced pa = produce(w, a, reads, 0xFFFFFFFFu, 4, 0);
    // b has handed nothing over, a's records wait for the workers: b's word shows them
    uint32_t seen_b = 0;
    const bool shown = wait_until([&] { seen_b = __atomic_load_n(&rb.ctl[0], __ATOMIC_ACQUIRE); return seen_b > 0; }, 30.0);
    { std::lock_guard<std::mutex> g(b.tb->mu); CHECK(shown && b.tb->dispatched == 0, "the second launch's backlog word stayed 0 beside %u records of the first", n); }
    // ... and while they do, a read of b that asks under "a worker is idle" (limit 1) is refused on a's account
    uint32_t k = 0;
    const uint32_t pend_b = __atomic_load_n(&rb.ctl[0], __ATOMIC_ACQUIRE);
    const int rc = claim(rb, 200, 1u, k);
    CHECK(pend_b == 0 || rc == 1, "claimed under limit 1 with a backlog word of %u", pend_b);
    if (rc == 0) publish(w, b, k, b.serial0 + 199, 0, 1);  // (the word fell to 0 between the two looks: the record is b's and is mapped like any other)
    Produced pb = produce(w, b, cycle(w, 199, 3), 0xFFFFFFFFu, 4, 0);
    b.read_of.resize(200, 0);
    const uint32_t handed_b = pb.handed + (rc == 0 ? 1u : 0u);
    CHECK(host::tail_finish(b.tb, rb.cursor.load()) && host::tail_finish(a.tb, ra.cursor.load()), "tail_finish");
    CHECK(pa.handed == n && pb.handed == 199, "handed %u and %u", pa.handed, pb.handed);
    check_results(w, a, n, "two batches, first");
    check_results(w, b, handed_b, "two batches, second");
    CHECK(wait_until([] { return host::TailWorkers::instance().pending() == 0; }, 30.0), "tasks left in the pool");
    std::printf("two batches: the second launch's backlog word showed %u tasks of the first\n", seen_b);
}

int main(int argc, char** argv) {
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    if (argc < 2) { std::printf("usage: tail_ring_selftest INPUT [watchdog seconds]\n"); return 2; }
    alarm(argc > 2 ? (unsigned)std::atoi(argv[2]) : 240u);  // a dispatcher that never ends is a failure, not a hang of the suite
    World w;
    if (!load(argv[1], w.in) || w.in.n_reads < 40) { std::printf("cannot read %s\n", argv[1]); return 2; }
    prepare(w);
    if (g_failed) return 1;
    CHECK(host::TailWorkers::instance().size() == 4, "MAPAD_TAIL_THREADS=4 is expected, the pool has %u", host::TailWorkers::instance().size());
    case_every_record(w);
    case_limit(w, 3);
    case_limit(w, 1);
    case_limit(w, 0);
    case_generations(w);
    case_clamp(w);
    case_cancel(w);
    case_two_batches(w);
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("tail ring selftest ok\n");
    return 0;
}
