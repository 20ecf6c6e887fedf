// abi_merge.hpp — fragment of mapad_amd.hip (host half; not a stand-alone header): adapter trimming and read-pair merging: mapad_merger, its device and host
// paths and its ABI.  Relies on k_merge.hpp, on lib_buffers.hpp (HIP_TRY, DevBuf, DevEvent) and, of mapad_amd.hip, on zero_async and kScanTile (the collect
// section); it needs no mapad_ctx.

// ---- adapter trimming and read-pair merging --------------------------------------------------------------------------------
namespace {
struct MergeResultOwner {
    mapad_merge_result_t r{};  // first: the handle is a pointer to it
    std::vector<uint8_t> cls, seqs, quals;
    std::vector<int32_t> frag_len;
    std::vector<uint16_t> m, x;
    std::vector<uint64_t> offsets;
    void room(uint64_t n) { cls.resize(n); frag_len.resize(n); m.resize(n); x.resize(n); offsets.resize(n + 1); }
    mapad_merge_result_t* publish(uint64_t n) {
        r.n_pairs = n; r.total_bases = offsets[n];
        r.cls = cls.data(); r.frag_len = frag_len.data(); r.matches = m.data(); r.mismatches = x.data();
        r.seqs = seqs.data(); r.quals = quals.data(); r.offsets = offsets.data();
        return &r;
    }
};
merge::Rule merge_rule(const mapad_merge_params_t& p) {
    merge::Rule R{};
    const bool single = p.mode == merge::MODE_SINGLE;
    R.min_overlap = single ? p.min_adapter_overlap : p.min_overlap;
    R.max_mismatch_permille = p.max_mismatch_permille; R.min_length = p.min_length; R.max_quality = p.max_quality; R.mode = p.mode;
    R.a1_len = p.adapter1_len; R.a2_len = single ? 0u : p.adapter2_len;
    std::memcpy(R.a1, p.adapter1, R.a1_len);
    std::memcpy(R.a2, p.adapter2, R.a2_len);
    return R;
}
void merge_counts_add(mapad_merge_counts_t& dst, const mapad_merge_counts_t& src) { mapad_merge_counts_add(&dst, &src); }
void merge_threads(uint64_t n, const std::function<void(uint64_t, uint64_t, unsigned)>& fn) {  // contiguous ranges on the process's share of the CPUs
    const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(host::cpu_share(), (n + 1023) / 1024));
    if (T == 1) { fn(0, n, 0); return; }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t) th.emplace_back(fn, n * t / T, n * (t + 1) / T, t);
    for (auto& t : th) t.join();
}
int merge_host(const mapad_merge_params_t* params, uint32_t mode, const uint8_t* seqs1, const uint8_t* quals1, const uint64_t* offs1, const uint8_t* seqs2,
               const uint8_t* quals2, const uint64_t* offs2, uint64_t n, mapad_merge_result_t** out) {
    if (!params || !out || params->mode != mode || mapad_merge_params_check(params)) return MAPAD_ERR_INVALID;
    const bool pairs = mode == merge::MODE_PAIRS;
    if (n && (!seqs1 || !quals1 || !offs1 || (pairs && (!seqs2 || !quals2 || !offs2)))) return MAPAD_ERR_INVALID;
    try {
        const merge::Rule R = merge_rule(*params);
        auto o = std::make_unique<MergeResultOwner>();
        o->room(n);
        std::vector<uint32_t> len(n);
        auto lens = [&](uint64_t r, int& L1, int& L2) {
            L1 = (int)std::min<uint64_t>(offs1[r + 1] - offs1[r], 0x7FFFFFFFull);
            L2 = pairs ? (int)std::min<uint64_t>(offs2[r + 1] - offs2[r], 0x7FFFFFFFull) : 0;
        };
        merge_threads(n, [&](uint64_t lo, uint64_t hi, unsigned) {
            for (uint64_t r = lo; r < hi; ++r) {
                int L1, L2;
                lens(r, L1, L2);
                const merge::Decision D = merge::decide(R, seqs1 + offs1[r], L1, pairs ? seqs2 + offs2[r] : nullptr, L2);
                o->cls[r] = (uint8_t)D.cls; o->frag_len[r] = D.frag_len; o->m[r] = (uint16_t)D.m; o->x[r] = (uint16_t)D.x; len[r] = (uint32_t)D.out_len;
            }
        });
        o->offsets[0] = 0;
        for (uint64_t r = 0; r < n; ++r) o->offsets[r + 1] = o->offsets[r] + len[r];
        o->seqs.resize(o->offsets[n]); o->quals.resize(o->offsets[n]);
        std::mutex mu;
        mapad_merge_counts_t& total = o->r.counts;
        merge_threads(n, [&](uint64_t lo, uint64_t hi, unsigned) {
            auto c = std::make_unique<mapad_merge_counts_t>();
            for (uint64_t r = lo; r < hi; ++r) {
                int L1, L2;
                lens(r, L1, L2);
                const int F = pairs ? o->frag_len[r] : (int)len[r];
                uint8_t* bs = o->seqs.data() + o->offsets[r];
                uint8_t* qs = o->quals.data() + o->offsets[r];
                for (int p = 0; p < (int)len[r]; ++p)
                    merge::column(R, seqs1 + offs1[r], quals1 + offs1[r], L1, pairs ? seqs2 + offs2[r] : nullptr, pairs ? quals2 + offs2[r] : nullptr, L2, F, p, bs[p], qs[p]);
                c->class_counts[o->cls[r]] += 1;
                c->bases_in += (offs1[r + 1] - offs1[r]) + (pairs ? offs2[r + 1] - offs2[r] : 0);
                c->bases_out += len[r];
                if (merge::yields_read(R, o->cls[r]) && len[r] < MAPAD_MERGE_HIST_BINS) c->histogram[len[r]] += 1;
            }
            c->pairs_seen = hi - lo;
            std::lock_guard<std::mutex> g(mu);
            merge_counts_add(total, *c);
        });
        total.calls = 1;
        *out = o.release()->publish(n);
        return MAPAD_OK;
    } catch (const std::bad_alloc&) { return MAPAD_ERR_NOMEM; }
}
}  // namespace

struct mapad_merger {
    int device = 0;
    mapad_merge_params_t params{};
    merge::Rule rule{};
    hipStream_t own = nullptr;     // non-blocking, created with the merger: its work waits for nobody's NULL-stream work and holds nobody's up
    hipStream_t stream = nullptr;  // `own`, or the caller's (mapad_merger_set_stream)
    DevBuf<uint8_t> d_seqs1, d_quals1, d_seqs2, d_quals2, d_cls, d_out_seqs, d_out_quals;
    DevBuf<uint64_t> d_offs1, d_offs2, d_out_offs;
    DevBuf<int32_t> d_frag;
    DevBuf<uint16_t> d_m, d_x;
    DevBuf<uint32_t> d_len;
    DevBuf<unsigned long long> d_tiles, d_counters;
    DevEvent ev[4];
    mapad_merge_counts_t totals{};
    MergeDev Q{};  // of the last call
};

namespace {
// decide, scan, (wait for the total), write: everything on m->stream; the inputs are device pointers.  `counts` gets this call's counters (the call waits for them)
int merge_run_device(mapad_merger* m, const uint8_t* s1, const uint8_t* q1, const uint64_t* o1, const uint8_t* s2, const uint8_t* q2, const uint64_t* o2, uint64_t n,
                     uint64_t& total, mapad_merge_counts_t& counts, float ms[2]) {
    int rc;
    hipStream_t st = m->stream;
    const uint64_t n_tiles = (n + kScanTile - 1) / kScanTile;
    if ((rc = m->d_cls.ensure(n)) || (rc = m->d_frag.ensure(n)) || (rc = m->d_m.ensure(n)) || (rc = m->d_x.ensure(n)) || (rc = m->d_len.ensure(n)) ||
        (rc = m->d_out_offs.ensure(n + 1)) || (rc = m->d_tiles.ensure(n_tiles + 1)) || (rc = m->d_counters.ensure(kMergeCounters, true))) return rc;
    for (auto& e : m->ev) if ((rc = e.ensure())) return rc;
    MergeDev& Q = m->Q;
    Q = MergeDev{};
    Q.R = m->rule;
    Q.seqs1 = s1; Q.quals1 = q1; Q.offs1 = o1; Q.seqs2 = s2; Q.quals2 = q2; Q.offs2 = o2; Q.n_pairs = n;
    Q.cls = m->d_cls.p; Q.frag_len = m->d_frag.p; Q.m = m->d_m.p; Q.x = m->d_x.p; Q.out_len = m->d_len.p; Q.out_offs = m->d_out_offs.p; Q.tile_sums = m->d_tiles.p;
    Q.counters = m->d_counters.p;
    if ((rc = zero_async(st, Q.counters, kMergeCounters * sizeof(unsigned long long)))) return rc;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kMergeBlock / 64 - 1) / (kMergeBlock / 64), 1u << 16);
    // the write kernel ends every block with a flush of its histogram and every wavefront with its counters' atomics: a grid of eight blocks per CU of a 256-CU
    // device keeps that to a few thousand flushes whatever the batch (the loop over pairs is grid-stride)
    const uint32_t grid_write = std::min<uint32_t>(grid, 2048u);
    HIP_TRY(hipEventRecord(m->ev[0], st));
    if (n) {
        hipLaunchKernelGGL(merge_decide_kernel, dim3(grid), dim3(kMergeBlock), 0, st, Q);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(m->ev[1], st));
    if (n) hipLaunchKernelGGL(merge_sums_kernel, dim3((uint32_t)n_tiles), dim3(64), 0, st, Q);
    hipLaunchKernelGGL(merge_scan_tiles_kernel, dim3(1), dim3(64), 0, st, Q, n_tiles);
    if (n) hipLaunchKernelGGL(merge_offsets_kernel, dim3((uint32_t)n_tiles), dim3(64), 0, st, Q);
    HIP_TRY(hipGetLastError());
    total = 0;
    HIP_TRY(hipMemcpyAsync(&total, Q.out_offs + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = m->d_out_seqs.ensure(total)) || (rc = m->d_out_quals.ensure(total))) return rc;
    Q.out_seqs = m->d_out_seqs.p; Q.out_quals = m->d_out_quals.p;
    HIP_TRY(hipEventRecord(m->ev[2], st));
    if (n) {
        hipLaunchKernelGGL(merge_write_kernel, dim3(grid_write), dim3(kMergeBlock), 0, st, Q);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(m->ev[3], st));
    std::vector<unsigned long long> h(kMergeCounters);
    HIP_TRY(hipMemcpyAsync(h.data(), Q.counters, kMergeCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&ms[0], m->ev[0], m->ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms[1], m->ev[2], m->ev[3]));
    counts = mapad_merge_counts_t{};
    counts.pairs_seen = n; counts.calls = 1;
    for (uint32_t k = 0; k < merge::N_CLASSES; ++k) counts.class_counts[k] = h[k];
    counts.bases_in = h[kMergeBasesIn]; counts.bases_out = h[kMergeBasesOut];
    for (int k = 0; k < MAPAD_MERGE_HIST_BINS; ++k) counts.histogram[k] = h[kMergeHist + k];
    merge_counts_add(m->totals, counts);
    return MAPAD_OK;
}
template <class T>
int merge_upload(hipStream_t st, DevBuf<T>& d, const T* h, uint64_t n) {
    int rc;
    if ((rc = d.ensure(n))) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(d.p, h, n * sizeof(T), hipMemcpyHostToDevice, st));
    return MAPAD_OK;
}
int merge_from_host_queued(mapad_merger* m, MergeResultOwner* o, bool pairs, const uint8_t* seqs1, const uint8_t* quals1, const uint64_t* offs1, const uint8_t* seqs2,
                           const uint8_t* quals2, const uint64_t* offs2, uint64_t n);
int merge_from_host(mapad_merger* m, uint32_t mode, const uint8_t* seqs1, const uint8_t* quals1, const uint64_t* offs1, const uint8_t* seqs2, const uint8_t* quals2,
                    const uint64_t* offs2, uint64_t n, mapad_merge_result_t** out) {
    if (!m || !out || m->params.mode != mode) return MAPAD_ERR_INVALID;
    const bool pairs = mode == merge::MODE_PAIRS;
    if (n && (!seqs1 || !quals1 || !offs1 || (pairs && (!seqs2 || !quals2 || !offs2)))) return MAPAD_ERR_INVALID;
    if (n >= 0xFFFFFFF0ull) return MAPAD_ERR_INVALID;
    if (hipSetDevice(m->device) != hipSuccess) return MAPAD_ERR_NO_DEVICE;
    try {
        auto o = std::make_unique<MergeResultOwner>();
        const int rc = merge_from_host_queued(m, o.get(), pairs, seqs1, quals1, offs1, seqs2, quals2, offs2, n);
        if (rc) { (void)hipStreamSynchronize(m->stream); return rc; }  // nothing queued may still read the caller's arrays or write into `o` once this returns
        *out = o.release()->publish(n);
        return MAPAD_OK;
    } catch (const std::bad_alloc&) { (void)hipStreamSynchronize(m->stream); return MAPAD_ERR_NOMEM; }
}
// uploads, the five launches, the copies back into `o`; returns with the stream drained on success.  On an error return work may still be queued: the caller waits
int merge_from_host_queued(mapad_merger* m, MergeResultOwner* o, bool pairs, const uint8_t* seqs1, const uint8_t* quals1, const uint64_t* offs1, const uint8_t* seqs2,
                           const uint8_t* quals2, const uint64_t* offs2, uint64_t n) {
    int rc;
    hipStream_t st = m->stream;
    static const uint64_t zero = 0;
    const uint64_t b1 = n ? offs1[n] : 0, b2 = (n && pairs) ? offs2[n] : 0;
    if ((rc = merge_upload(st, m->d_seqs1, seqs1, b1)) || (rc = merge_upload(st, m->d_quals1, quals1, b1)) || (rc = merge_upload(st, m->d_offs1, n ? offs1 : &zero, n + 1))) return rc;
    if (pairs && ((rc = merge_upload(st, m->d_seqs2, seqs2, b2)) || (rc = merge_upload(st, m->d_quals2, quals2, b2)) || (rc = merge_upload(st, m->d_offs2, n ? offs2 : &zero, n + 1)))) return rc;
    uint64_t total = 0;
    if ((rc = merge_run_device(m, m->d_seqs1.p, m->d_quals1.p, m->d_offs1.p, pairs ? m->d_seqs2.p : nullptr, pairs ? m->d_quals2.p : nullptr, pairs ? m->d_offs2.p : nullptr, n,
                               total, o->r.counts, o->r.kernel_ms))) return rc;
    o->room(n);
    o->seqs.resize(total); o->quals.resize(total);
    if (n) {
        HIP_TRY(hipMemcpyAsync(o->cls.data(), m->d_cls.p, n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(o->frag_len.data(), m->d_frag.p, n * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(o->m.data(), m->d_m.p, n * 2, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(o->x.data(), m->d_x.p, n * 2, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(o->offsets.data(), m->d_out_offs.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (total) {
        HIP_TRY(hipMemcpyAsync(o->seqs.data(), m->d_out_seqs.p, total, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(o->quals.data(), m->d_out_quals.p, total, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MAPAD_OK;
}
}  // namespace

extern "C" {
void mapad_merge_params_default(mapad_merge_params_t* out) {
    if (!out) return;
    static const char a1[] = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", a2[] = "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT";
    *out = mapad_merge_params_t{};
    out->min_overlap = 11; out->min_adapter_overlap = 3; out->max_mismatch_permille = 166; out->min_length = 15; out->max_quality = 41;
    out->adapter1_len = sizeof a1 - 1; out->adapter2_len = sizeof a2 - 1;
    std::memcpy(out->adapter1, a1, sizeof a1 - 1);
    std::memcpy(out->adapter2, a2, sizeof a2 - 1);
}
int mapad_merge_params_check(const mapad_merge_params_t* p) {
    if (!p) return MAPAD_ERR_INVALID;
    if (p->adapter1_len > MAPAD_MERGE_MAX_ADAPTER || p->adapter2_len > MAPAD_MERGE_MAX_ADAPTER) return MAPAD_ERR_INVALID;
    for (uint32_t k = 0; k < p->adapter1_len; ++k) if (!merge::valid_base(p->adapter1[k])) return MAPAD_ERR_INVALID;
    for (uint32_t k = 0; k < p->adapter2_len; ++k) if (!merge::valid_base(p->adapter2[k])) return MAPAD_ERR_INVALID;
    if (p->min_overlap < 1 || p->min_adapter_overlap < 1 || p->max_quality > 93 || p->max_mismatch_permille > 1000 || p->mode > 1) return MAPAD_ERR_INVALID;
    return MAPAD_OK;
}
int mapad_merger_create(int device_id, const mapad_merge_params_t* params, mapad_merger_t** out) {
    if (!params || !out) return MAPAD_ERR_INVALID;
    int rc;
    if ((rc = mapad_merge_params_check(params))) return rc;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device_id < 0 || device_id >= n_dev) {
        std::fprintf(stderr, "mapad_amd: no usable HIP device (mapad_merge_pairs_host is the host path of this stage)\n");
        return MAPAD_ERR_NO_DEVICE;
    }
    if (hipSetDevice(device_id) != hipSuccess) return MAPAD_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return MAPAD_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::fprintf(stderr, "mapad_amd: device %d is %s, this library is built for gfx950 only\n", device_id, prop.gcnArchName);
        return MAPAD_ERR_NO_DEVICE;
    }
    auto m = std::make_unique<mapad_merger>();
    m->device = device_id; m->params = *params; m->rule = merge_rule(*params);
    HIP_TRY(hipStreamCreateWithFlags(&m->own, hipStreamNonBlocking));
    m->stream = m->own;
    *out = m.release();
    return MAPAD_OK;
}
int mapad_merger_set_stream(mapad_merger_t* m, void* s) { if (!m) return MAPAD_ERR_INVALID; m->stream = s ? (hipStream_t)s : m->own; return MAPAD_OK; }
void mapad_merger_free(mapad_merger_t* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);  // the buffers free themselves on the merger's device
    if (m->own) { (void)hipStreamSynchronize(m->own); (void)hipStreamDestroy(m->own); }
    delete m;
}
int mapad_merge_pairs(mapad_merger_t* m, const uint8_t* seqs1, const uint8_t* quals1, const uint64_t* offsets1, const uint8_t* seqs2, const uint8_t* quals2,
                      const uint64_t* offsets2, uint64_t n_pairs, mapad_merge_result_t** out) {
    return merge_from_host(m, merge::MODE_PAIRS, seqs1, quals1, offsets1, seqs2, quals2, offsets2, n_pairs, out);
}
int mapad_trim_reads(mapad_merger_t* m, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n, mapad_merge_result_t** out) {
    return merge_from_host(m, merge::MODE_SINGLE, seqs, quals, offsets, nullptr, nullptr, nullptr, n, out);
}
void mapad_merge_result_free(mapad_merge_result_t* r) { delete reinterpret_cast<MergeResultOwner*>(r); }
void mapad_merge_counts_add(mapad_merge_counts_t* dst, const mapad_merge_counts_t* src) {
    if (!dst || !src) return;
    dst->pairs_seen += src->pairs_seen; dst->bases_in += src->bases_in; dst->bases_out += src->bases_out; dst->calls += src->calls;
    for (int k = 0; k < MAPAD_MERGE_CLASSES; ++k) dst->class_counts[k] += src->class_counts[k];
    for (int k = 0; k < MAPAD_MERGE_HIST_BINS; ++k) dst->histogram[k] += src->histogram[k];
}
int mapad_merger_totals(mapad_merger_t* m, mapad_merge_counts_t* out) { if (!m || !out) return MAPAD_ERR_INVALID; *out = m->totals; return MAPAD_OK; }
int mapad_merger_reset(mapad_merger_t* m) { if (!m) return MAPAD_ERR_INVALID; m->totals = mapad_merge_counts_t{}; return MAPAD_OK; }
int mapad_merge_pairs_device(mapad_merger_t* m, const void* d_seqs1, const void* d_quals1, const void* d_offsets1, const void* d_seqs2, const void* d_quals2,
                             const void* d_offsets2, uint64_t n_pairs, void** d_seqs, void** d_quals, void** d_offsets, uint64_t* total_bases) {
    if (!m || !d_seqs || !d_quals || !d_offsets || !total_bases) return MAPAD_ERR_INVALID;
    const bool pairs = m->params.mode == merge::MODE_PAIRS;
    if (n_pairs && (!d_seqs1 || !d_quals1 || !d_offsets1 || (pairs && (!d_seqs2 || !d_quals2 || !d_offsets2)))) return MAPAD_ERR_INVALID;
    if (n_pairs >= 0xFFFFFFF0ull) return MAPAD_ERR_INVALID;
    if (hipSetDevice(m->device) != hipSuccess) return MAPAD_ERR_NO_DEVICE;
    try {
        mapad_merge_counts_t counts;
        float ms[2];
        const int rc = merge_run_device(m, (const uint8_t*)d_seqs1, (const uint8_t*)d_quals1, (const uint64_t*)d_offsets1, pairs ? (const uint8_t*)d_seqs2 : nullptr,
                                        pairs ? (const uint8_t*)d_quals2 : nullptr, pairs ? (const uint64_t*)d_offsets2 : nullptr, n_pairs, *total_bases, counts, ms);
        if (rc) { (void)hipStreamSynchronize(m->stream); return rc; }  // nothing queued may still read the caller's buffers
        *d_seqs = m->d_out_seqs.p; *d_quals = m->d_out_quals.p; *d_offsets = m->d_out_offs.p;
        return MAPAD_OK;
    } catch (const std::bad_alloc&) { return MAPAD_ERR_NOMEM; }
}
int mapad_merge_pairs_host(const mapad_merge_params_t* params, const uint8_t* seqs1, const uint8_t* quals1, const uint64_t* offsets1, const uint8_t* seqs2,
                           const uint8_t* quals2, const uint64_t* offsets2, uint64_t n_pairs, mapad_merge_result_t** out) {
    return merge_host(params, merge::MODE_PAIRS, seqs1, quals1, offsets1, seqs2, quals2, offsets2, n_pairs, out);
}
int mapad_trim_reads_host(const mapad_merge_params_t* params, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n, mapad_merge_result_t** out) {
    return merge_host(params, merge::MODE_SINGLE, seqs, quals, offsets, nullptr, nullptr, nullptr, n, out);
}
}  // extern "C"
