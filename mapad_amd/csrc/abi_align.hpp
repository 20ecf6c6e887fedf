// abi_align.hpp — fragment of mapad_amd.hip (host half; not a stand-alone header): the stages over existing alignments: build_tracks,
// mapad_ctx_accumulate_alignments, the tracks' read-outs and their host mirror.  Relies on k_align.hpp, on lib_buffers.hpp (HIP_TRY) and on what mapad_amd.hip
// defines in front of it: mapad_ctx, BatchSlot, BatchDev and the cursors (CUR_COUNT); zero_async, read_back_words; the collect section (kScanTile, CompactDev,
// compact_sums_kernel, compact_scan_tiles_kernel); the stages' launch side (StageArgs, grid_for, kStageLaunch, launch_dedup); the pipeline (acquire_slot,
// upload_tables, next_launch_serial) and stage_host_batch.

extern "C" {

// ---- the stages over existing alignments (align_core.hpp; align_count_kernel, align_build_kernel) ----
namespace {
static_assert(sizeof(mapad_alignment_t) == sizeof(AlignIn) && offsetof(mapad_alignment_t, tid) == offsetof(AlignIn, tid) && offsetof(mapad_alignment_t, flags) == offsetof(AlignIn, flags) &&
                  offsetof(mapad_alignment_t, mapq) == offsetof(AlignIn, mapq) && offsetof(mapad_alignment_t, md_len) == offsetof(AlignIn, md_len),
              "alignment records are copied as they are");
static_assert(MAPAD_ALN_CLASSES == ALN_CLASSES, "status classes");
struct AlnResultOwner {
    mapad_aln_result_t pub{};  // first member: the public pointer is the object's
    std::vector<uint8_t> cls, dup, scored, rescaled;
    std::vector<int32_t> score_q;
};
struct TracksOwner {
    mapad_tracks_t pub{};
    std::vector<uint64_t> hit_begin, x0, rel, abs;
    std::vector<HitRec> hits;
    std::vector<uint32_t> ops, mapped, error, best, backward;
    std::vector<int32_t> tid;
    std::vector<uint8_t> cls;
    void resize(uint64_t n, uint64_t n_ops) {
        hit_begin.resize(n + 1); hits.resize(n); ops.resize(n_ops); cls.resize(n);
        mapped.resize(n); error.resize(n); best.resize(n); x0.resize(n); tid.resize(n); rel.resize(n); abs.resize(n); backward.resize(n);
    }
    void set(uint64_t r, const CoordRec& cr) {
        mapped[r] = cr.mapped; error[r] = cr.error; best[r] = cr.best; x0[r] = cr.x0; tid[r] = cr.first.tid; rel[r] = cr.first.rel; abs[r] = cr.first.abs; backward[r] = cr.first.backward;
    }
    mapad_tracks_t* publish() {
        static_assert(sizeof(mapad_hit_t) == sizeof(HitRec), "hit records are handed out as they are");
        pub.n_reads = hits.size(); pub.n_ops = ops.size();
        pub.hit_begin = hit_begin.data(); pub.hits = reinterpret_cast<const mapad_hit_t*>(hits.data()); pub.ops = ops.data(); pub.status_class = cls.data();
        pub.mapped = mapped.data(); pub.error = error.data(); pub.best = best.data(); pub.x0 = x0.data(); pub.tid = tid.data(); pub.rel = rel.data(); pub.abs = abs.data();
        pub.backward = backward.data();
        for (auto& c : pub.class_counts) c = 0;
        for (uint8_t c : cls) if (c < ALN_CLASSES) pub.class_counts[c] += 1;
        return &pub;
    }
};
// how far the records reach into the two arrays they point into; false: a record's end does not fit 64 bits
bool align_extents(const mapad_alignment_t* alns, uint64_t n, uint64_t& n_cigar, uint64_t& n_md) {
    n_cigar = 0; n_md = 0;
    for (uint64_t r = 0; r < n; ++r) {
        const mapad_alignment_t& a = alns[r];
        if (a.cigar_off > (1ull << 62) || a.md_off > (1ull << 62)) return false;
        if (a.n_cigar) n_cigar = std::max<uint64_t>(n_cigar, a.cigar_off + a.n_cigar);
        if (a.md_len) n_md = std::max<uint64_t>(n_md, a.md_off + a.md_len);
    }
    return true;
}
void contig_table(const host::Index& ix, std::vector<uint64_t>& cs) {  // starts, then inclusive ends
    cs.clear();
    for (auto& k : ix.contigs) cs.push_back(k.start);
    for (auto& k : ix.contigs) cs.push_back(k.end);
}
// the tracks of the slot's batch on S.stream: count, scan, build (between ctx->ev_an); S.c_n_ops = the ops array's words.  Synchronises the stream once, for the total.
int build_tracks(mapad_ctx* c, BatchSlot& S, uint64_t n, const mapad_alignment_t* alns, const uint32_t* cigar_words, uint64_t n_cigar, const uint8_t* md_bytes, uint64_t n_md,
                 uint32_t min_mapq) {
    const host::Index& ix = c->index->ix;
    int rc;
    if (!c->d_an_contigs.cap) {
        std::vector<uint64_t> cs;
        contig_table(ix, cs);
        if ((rc = c->d_an_contigs.ensure(std::max<size_t>(cs.size(), 2), true))) return rc;
        if (!cs.empty()) HIP_TRY(hipMemcpy(c->d_an_contigs.p, cs.data(), cs.size() * 8, hipMemcpyHostToDevice));
    }
    const uint64_t n_tiles = (n + kScanTile - 1) / kScanTile;
    if ((rc = S.d_an_in.ensure(n))) return rc;
    if ((rc = S.d_an_cigar.ensure(std::max<uint64_t>(n_cigar, 1)))) return rc;
    if ((rc = S.d_an_md.ensure(std::max<uint64_t>(n_md, 1)))) return rc;
    if ((rc = S.d_an_cls.ensure(n))) return rc;
    if ((rc = S.d_hit_count.ensure(n))) return rc;
    if ((rc = S.d_hit_first.ensure(n))) return rc;
    if ((rc = S.d_c_hit_begin.ensure(n + 1))) return rc;
    if ((rc = S.d_c_ops_begin.ensure(n + 1))) return rc;
    if ((rc = S.d_c_tiles.ensure(2 * n_tiles))) return rc;
    if ((rc = S.d_c_hits.ensure(n))) return rc;
    if ((rc = S.d_rec_coords.ensure(n))) return rc;
    if ((rc = c->d_an_cnt.ensure(ALN_CLASSES))) return rc;
    if (!S.h_small.resize(CUR_COUNT + 8)) return MAPAD_ERR_NOMEM;
    for (auto& e : c->ev_an) if (e.ensure()) return MAPAD_ERR_DEVICE;
    HIP_TRY(hipMemcpyAsync(S.d_an_in.p, alns, n * sizeof(AlignIn), hipMemcpyHostToDevice, S.stream));
    if (n_cigar) HIP_TRY(hipMemcpyAsync(S.d_an_cigar.p, cigar_words, n_cigar * 4, hipMemcpyHostToDevice, S.stream));
    if (n_md) HIP_TRY(hipMemcpyAsync(S.d_an_md.p, md_bytes, n_md, hipMemcpyHostToDevice, S.stream));
    if ((rc = zero_async(S.stream, c->d_an_cnt.p, ALN_CLASSES * 8))) return rc;
    AlignDev Q{};
    Q.alns = S.d_an_in.p; Q.cigar = S.d_an_cigar.p; Q.md = S.d_an_md.p; Q.offsets = S.last.offsets; Q.n_reads = n;
    Q.contig_start = c->d_an_contigs.p; Q.contig_end = c->d_an_contigs.p + ix.contigs.size(); Q.n_contigs = (uint32_t)ix.contigs.size(); Q.min_mapq = min_mapq;
    Q.start_at_end = c->params.model_kind == MAPAD_MODEL_SIMPLE_ADNA ? 1u : 0u;
    Q.hit_count = S.d_hit_count.p; Q.hit_first = S.d_hit_first.p; Q.hit_begin = S.d_c_hit_begin.p; Q.ops_begin = S.d_c_ops_begin.p; Q.hits = S.d_c_hits.p; Q.ops = nullptr;
    Q.coords = S.d_rec_coords.p; Q.cls = S.d_an_cls.p; Q.counters = c->d_an_cnt.p;
    HIP_TRY(hipEventRecord(c->ev_an[0], S.stream));
    hipLaunchKernelGGL(align_count_kernel, dim3(grid_for(n, kAlignBlock, c)), dim3(kAlignBlock), 0, S.stream, Q);
    HIP_TRY(hipGetLastError());
    CompactDev CQ{S.d_hit_count.p, S.d_hit_first.p, S.d_c_hits.p, nullptr, n, S.d_c_hit_begin.p, S.d_c_ops_begin.p, S.d_c_tiles.p, S.d_c_tiles.p + n_tiles, nullptr, nullptr};
    hipLaunchKernelGGL(compact_sums_kernel, dim3((uint32_t)n_tiles), dim3(64), 0, S.stream, CQ);
    hipLaunchKernelGGL(compact_scan_tiles_kernel, dim3(1), dim3(64), 0, S.stream, CQ, n_tiles);
    hipLaunchKernelGGL(align_begin_kernel, dim3((uint32_t)n_tiles), dim3(64), 0, S.stream, Q, (const unsigned long long*)(S.d_c_tiles.p + n_tiles));
    HIP_TRY(hipGetLastError());
    if ((rc = read_back_words(S.stream, S.d_c_ops_begin.p + n, S.h_small, CUR_COUNT, 2))) return rc;
    uint64_t total = 0;
    std::memcpy(&total, S.h_small.data() + CUR_COUNT, 8);
    if (total > 0xFFFFFFFFull) {  // (a hit's ops_off is 32 bits wide)
        std::fprintf(stderr, "mapad_amd: the batch's alignments have more than 2^32 edit operations; split it\n");
        return MAPAD_ERR_INVALID;
    }
    if ((rc = S.d_c_ops.ensure(std::max<uint64_t>(total, 1)))) return rc;
    Q.ops = S.d_c_ops.p;
    hipLaunchKernelGGL(align_build_kernel, dim3(grid_for(n, kAlignBlock / 64, c)), dim3(kAlignBlock), 0, S.stream, Q);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_an[1], S.stream));
    S.c_n_hits = n; S.c_n_ops = total;
    return MAPAD_OK;
}
}  // namespace

int mapad_ctx_accumulate_alignments(mapad_ctx_t* ctx, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n_reads, const mapad_alignment_t* alns,
                                    const uint32_t* cigar_words, const uint8_t* md_bytes, uint32_t min_mapq, mapad_aln_result_t** out) {
    if (!ctx || !out || min_mapq > 255 || (n_reads && (!seqs || !quals || !offsets || !alns))) return MAPAD_ERR_INVALID;
    if (n_reads >= 0xFFFFFFF0ull) return MAPAD_ERR_INVALID;
    uint64_t n_cigar = 0, n_md = 0;
    if (!align_extents(alns, n_reads, n_cigar, n_md) || (n_cigar && !cigar_words) || (n_md && !md_bytes)) return MAPAD_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return MAPAD_ERR_NO_DEVICE;
    try {
        int rc;
        if ((rc = acquire_slot(ctx, (ctx->cur + 1) % ctx->depth))) return rc;
        BatchSlot& S = ctx->bs[ctx->cur];
        uint64_t total = 0;
        uint32_t lmax = 0;
        if ((rc = stage_host_batch(ctx, S, seqs, quals, offsets, n_reads, total, lmax))) return rc;  // (with the score tables of the batch's lengths)
        if ((rc = upload_tables(ctx))) return rc;
        // the slot holds this batch now — its reads, nothing of a search: no D arrays, no arenas, no pools
        BatchDev B{};
        B.seqs = S.d_seqs.p; B.quals = S.d_quals.p; B.offsets = S.d_offsets.p; B.n_reads = (uint32_t)n_reads; B.tail_pops = 0xFFFFFFFFu;
        S.last = B; S.last_total_bases = total; S.last_lmax = lmax; S.compacted = false; S.collapsed = false; S.fan_done = false; S.c_stats = nullptr;
        S.ev_valid = false; S.timed = true; S.tail_failed = false; S.c_n_hits = 0; S.c_n_ops = 0;
        S.gen = next_launch_serial(); S.aligned = false;  // (set once the tracks stand and the stages have run: a failed call leaves a slot that holds no batch)
        S.last.n_reads = 0;  // (an empty slot to every other entry point until then)
        auto r = std::make_unique<AlnResultOwner>();
        r->pub.n_reads = n_reads;
        if (n_reads == 0) {  // nothing to build; with duplicates marked, the empty batch still counts as one (as an empty batch converted to records does)
            if ((rc = launch_dedup(ctx, S, StageArgs{nullptr, nullptr, nullptr, nullptr, 0, S.stream}))) return rc;
            S.aligned = true;
            *out = &r.release()->pub;
            return MAPAD_OK;
        }
        // whatever fails from here on, the stream is waited for before the call's buffers go away (kernels and copies queued on it read and write them)
        struct Drain { hipStream_t st; bool armed = true; ~Drain() { if (armed) (void)hipStreamSynchronize(st); } } drain{S.stream};
        if ((rc = build_tracks(ctx, S, n_reads, alns, cigar_words, n_cigar, md_bytes, n_md, min_mapq))) return rc;
        for (StageLaunch launch : kStageLaunch)
            if ((rc = launch(ctx, S, StageArgs{S.d_c_hit_begin.p, S.d_c_hits.p, S.d_c_ops.p, S.d_rec_coords.p, n_reads, S.stream}))) return rc;
        unsigned long long counts[ALN_CLASSES] = {};
        r->cls.resize(n_reads);
        HIP_TRY(hipMemcpyAsync(r->cls.data(), S.d_an_cls.p, n_reads, hipMemcpyDeviceToHost, S.stream));
        HIP_TRY(hipMemcpyAsync(counts, ctx->d_an_cnt.p, sizeof counts, hipMemcpyDeviceToHost, S.stream));
        if (ctx->dedup_mode) {
            r->dup.resize(n_reads);
            HIP_TRY(hipMemcpyAsync(r->dup.data(), S.d_dup.p, n_reads, hipMemcpyDeviceToHost, S.stream));
        }
        if (ctx->dscore_mode) {
            r->score_q.resize(n_reads); r->scored.resize(n_reads);
            HIP_TRY(hipMemcpyAsync(r->score_q.data(), S.d_ds_score.p, n_reads * sizeof(int32_t), hipMemcpyDeviceToHost, S.stream));
            HIP_TRY(hipMemcpyAsync(r->scored.data(), S.d_ds_scored.p, n_reads, hipMemcpyDeviceToHost, S.stream));
        }
        if (ctx->rescale_mode) {
            r->rescaled.resize(std::max<uint64_t>(total, 1));
            if (total) HIP_TRY(hipMemcpyAsync(r->rescaled.data(), S.d_rs_quals.p, total, hipMemcpyDeviceToHost, S.stream));
        }
        HIP_TRY(hipStreamSynchronize(S.stream));
        drain.armed = false;
        S.last.n_reads = (uint32_t)n_reads; S.aligned = true;
        HIP_TRY(hipEventElapsedTime(&r->pub.build_ms, ctx->ev_an[0], ctx->ev_an[1]));
        for (uint32_t k = 0; k < ALN_CLASSES; ++k) r->pub.class_counts[k] = counts[k];
        r->pub.status_class = r->cls.data();
        r->pub.duplicate = ctx->dedup_mode ? r->dup.data() : nullptr;
        r->pub.scored = ctx->dscore_mode ? r->scored.data() : nullptr;
        r->pub.score_q = ctx->dscore_mode ? r->score_q.data() : nullptr;
        r->pub.rescaled_quals = ctx->rescale_mode ? r->rescaled.data() : nullptr;
        r->pub.n_quals = ctx->rescale_mode ? total : 0;
        *out = &r.release()->pub;
        return MAPAD_OK;
    } catch (const std::bad_alloc&) { return MAPAD_ERR_NOMEM; }
}
void mapad_aln_result_free(mapad_aln_result_t* r) { delete reinterpret_cast<AlnResultOwner*>(r); }

int mapad_ctx_alignment_tracks(mapad_ctx_t* ctx, mapad_tracks_t** out) {
    if (!ctx || !out) return MAPAD_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return MAPAD_ERR_NO_DEVICE;
    BatchSlot& S = ctx->bs[ctx->view];
    if (!S.aligned) return MAPAD_ERR_INVALID;  // the slot's batch did not come through mapad_ctx_accumulate_alignments
    try {
        const uint64_t n = S.last.n_reads;
        auto t = std::make_unique<TracksOwner>();
        t->resize(n, n ? S.c_n_ops : 0);
        std::vector<CoordRec> coords(n);
        if (n) {
            HIP_TRY(hipMemcpyAsync(t->hit_begin.data(), S.d_c_hit_begin.p, (n + 1) * 8, hipMemcpyDeviceToHost, S.stream));
            HIP_TRY(hipMemcpyAsync(t->hits.data(), S.d_c_hits.p, n * sizeof(HitRec), hipMemcpyDeviceToHost, S.stream));
            if (S.c_n_ops) HIP_TRY(hipMemcpyAsync(t->ops.data(), S.d_c_ops.p, S.c_n_ops * 4, hipMemcpyDeviceToHost, S.stream));
            HIP_TRY(hipMemcpyAsync(t->cls.data(), S.d_an_cls.p, n, hipMemcpyDeviceToHost, S.stream));
            HIP_TRY(hipMemcpyAsync(coords.data(), S.d_rec_coords.p, n * sizeof(CoordRec), hipMemcpyDeviceToHost, S.stream));
            HIP_TRY(hipStreamSynchronize(S.stream));
        } else t->hit_begin[0] = 0;
        for (uint64_t r = 0; r < n; ++r) t->set(r, coords[r]);
        *out = t.release()->publish();
        return MAPAD_OK;
    } catch (const std::bad_alloc&) { return MAPAD_ERR_NOMEM; }
}
int mapad_alignment_tracks_host(const mapad_index_t* idx, const mapad_params_t* params, const uint64_t* offsets, uint64_t n_reads, const mapad_alignment_t* alns,
                                const uint32_t* cigar_words, const uint8_t* md_bytes, uint32_t min_mapq, mapad_tracks_t** out) {
    if (!idx || !params || !out || min_mapq > 255 || (n_reads && (!offsets || !alns)) || n_reads >= 0xFFFFFFF0ull) return MAPAD_ERR_INVALID;
    uint64_t n_cigar = 0, n_md = 0;
    if (!align_extents(alns, n_reads, n_cigar, n_md) || (n_cigar && !cigar_words) || (n_md && !md_bytes)) return MAPAD_ERR_INVALID;
    try {
        std::vector<uint64_t> cs;
        contig_table(idx->ix, cs);
        const uint32_t n_contigs = (uint32_t)idx->ix.contigs.size();
        const bool start_at_end = params->model_kind == MAPAD_MODEL_SIMPLE_ADNA;
        const AlignIn* in = reinterpret_cast<const AlignIn*>(alns);
        // the count, then the scan (a read keeps the room its CIGAR asks for, whatever class it ends in), then the build: as on the device
        std::vector<uint64_t> begin(n_reads + 1, 0);
        for (uint64_t r = 0; r < n_reads; ++r) {
            const uint64_t L = offsets[r + 1] - offsets[r];
            if (L > MAPAD_MAX_READ_LEN) return MAPAD_ERR_READ_TOO_LONG;
            uint32_t n_ops;
            uint64_t ref_len;
            (void)align_count(in[r], cigar_words + in[r].cigar_off, L, n_contigs, min_mapq, n_ops, ref_len);
            begin[r + 1] = begin[r] + n_ops;
        }
        if (begin[n_reads] > 0xFFFFFFFFull) return MAPAD_ERR_INVALID;
        auto t = std::make_unique<TracksOwner>();
        t->resize(n_reads, begin[n_reads]);
        for (uint64_t r = 0; r <= n_reads; ++r) t->hit_begin[r] = r;
        for (uint64_t r = 0; r < n_reads; ++r) {
            CoordRec cr;
            t->cls[r] = (uint8_t)align_read(in[r], cigar_words, md_bytes, (uint32_t)(offsets[r + 1] - offsets[r]), cs.data(), cs.data() + n_contigs, n_contigs, min_mapq, start_at_end,
                                            (uint32_t)begin[r], t->ops.data(), t->hits[r], cr);
            t->set(r, cr);
        }
        *out = t.release()->publish();
        return MAPAD_OK;
    } catch (const std::bad_alloc&) { return MAPAD_ERR_NOMEM; }
}
void mapad_tracks_free(mapad_tracks_t* t) { delete reinterpret_cast<TracksOwner*>(t); }

}  // extern "C"
