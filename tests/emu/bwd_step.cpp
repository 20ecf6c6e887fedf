// bwd_step.cpp — TEST-ONLY host build of the search step with its direction chosen by the caller (search_core.hpp: search_step<.., BWD>).
//
// emu.cpp runs a batch through search_read, which picks the step by the model as the kernel launch does.  This entry point runs the same per-read loop with the
// backward-only step (direction 1), the general step (direction 0) or the dispatcher's choice (direction -1, reported back), so that the CPU suite can hold the
// two instantiations against each other read by read; the host build of the step asserts the invariant the backward-only one rests on at every pop.
// Built into tests/emu/_build by tests/test_bwd_step_host.py; never loaded by the product.
#include <algorithm>
#include <cstring>
#include <vector>

#define MAPAD_PAR_COMMIT_EMU 1  // the lane-parallel commit of the quad kernel, emulated lane by lane (runs when the payload cache is off)

#include "../../include/mapad_amd.h"
#include "../../mapad_amd/csrc/darray_core.hpp"
#include "../../mapad_amd/csrc/host_models.hpp"
#include "../../mapad_amd/csrc/search_core.hpp"

using namespace mapad;

namespace {
struct DirResult {
    mapad_batch_result_t pub{};
    std::vector<uint64_t> hit_begin;
    std::vector<mapad_hit_t> hits;
    std::vector<uint32_t> ops, status;
    std::vector<mapad_read_counters_t> counters;
    std::vector<float> d_arrays;
};
}  // namespace

extern "C" {

// direction: 1 = search_step<.., BWD = true>, 0 = the general step, -1 = what search_read chooses; payload_cache: the step's PC variant (as the host tail runs it)
// or the plain step with the emulated lane-parallel commit.  *chosen: 1 if the backward-only step ran.  Arenas with the reference's full limits, grown lazily.
mapad_batch_result_t* bwd_map_batch(const uint64_t* blocks, uint64_t n_blocks, uint64_t n, const uint64_t* less8, const uint64_t* sentinel2, const mapad_params_t* p,
                                    const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n_reads, int direction, int payload_cache, int* chosen) {
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
    const bool bwd = direction < 0 ? step_is_backward_only(P) : direction != 0;
    if (chosen) *chosen = bwd ? 1 : 0;

    auto* r = new DirResult();
    r->hit_begin.assign(n_reads + 1, 0); r->status.resize(n_reads); r->counters.resize(n_reads);
    r->d_arrays.resize(n_reads ? offsets[n_reads] : 0);
    std::vector<HeapEntry> top(kTop + 1 + 8);
    uint64_t pc_words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint8_t> qc(2 * (lmax + 1));
    std::vector<float> dnear(lmax + 1), pen(lmax + 1), chain(lmax + 1);
    const uint32_t hc = std::min<uint32_t>(P.stack_limit + 10, 1u << 22), nc = std::min<uint32_t>(P.edit_tree_limit + 10, 1u << 22);
    std::vector<HeapEntry> heap(std::max<size_t>(2 * (size_t)hc, HeapLayout<kTop>::phys_end(hc)) + 64);
    std::vector<Node> nodes(nc);
    std::vector<HitRec> hits(kMaxHits);
    std::vector<uint32_t> hit_ops(kMaxHits * (lmax + 32));
    std::vector<uint16_t> scratch(2 * (lmax + 2));
    for (uint64_t i = 0; i < n_reads; ++i) {
        const uint64_t off = offsets[i];
        const int L = (int)(offsets[i + 1] - off);
        float* d = r->d_arrays.data() + off;
        ReadCounters ctr{};
        ctr.e_darray = d_array_scalar(ix, P, seqs + off, quals + off, L, pen.data(), chain.data(), d);
        read_setup(seqs + off, quals + off, d, L, qc.data(), dnear.data(), 0, 1);
        Arena A;
        A.top = top.data() + 1; A.heap = heap.data() + 1; A.nodes = nodes.data(); A.hits = hits.data(); A.hit_ops = hit_ops.data(); A.scratch = scratch.data();
        A.heap_cap = hc; A.node_cap = nc; A.hit_ops_cap = (uint32_t)hit_ops.size();
        A.pc = payload_cache ? pc_words : nullptr;
        const ReadIn rd{qc.data(), dnear.data(), L, P.reject_thr[L], P.table_base[L]};
        SearchState st;
        if (direction < 0) search_read(ix, P, rd, A, st, 0);
        else if (bwd) search_read_dir<true>(ix, P, rd, A, st, 0);
        else search_read_dir<false>(ix, P, rd, A, st, 0);
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
    r->pub.n_reads = n_reads; r->pub.n_hits = r->hits.size(); r->pub.n_ops = r->ops.size();
    r->pub.hit_begin = r->hit_begin.data(); r->pub.hits = r->hits.data(); r->pub.ops = r->ops.data(); r->pub.status = r->status.data();
    r->pub.counters = r->counters.data(); r->pub.d_arrays = r->d_arrays.data(); r->pub.n_second_pass = 0; r->pub.n_third_pass = 0;
    return &r->pub;
}
void bwd_result_free(mapad_batch_result_t* r) { if (r) delete reinterpret_cast<DirResult*>(r); }

}  // extern "C"
