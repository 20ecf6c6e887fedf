// abi_clean.hpp — fragment of mapad_amd.hip (host half; not a stand-alone header): the read clean-up: mapad_cleaner, its device and host paths and its ABI.
// Relies on k_clean.hpp and k_merge.hpp (the scan launches), on abi_merge.hpp in front of it (merge_threads, merge_upload), on lib_buffers.hpp (HIP_TRY, DevBuf,
// DevEvent) and, of mapad_amd.hip, on zero_async and kScanTile (the collect section); it needs no mapad_ctx.

// ---- read clean-up ---------------------------------------------------------------------------------------------------------------------------------------------
namespace {
struct CleanResultOwner {
    mapad_clean_result_t r{};  // first: the handle is a pointer to it
    std::vector<uint8_t> cls, seqs, quals;
    std::vector<uint16_t> trim5, trim3, poly, dust;
    std::vector<uint64_t> offsets;
    void room(uint64_t n) { cls.resize(n); trim5.resize(n); trim3.resize(n); poly.resize(n); dust.resize(n); offsets.resize(n + 1); }
    mapad_clean_result_t* publish(uint64_t n) {
        r.n_reads = n; r.total_bases = offsets[n];
        r.cls = cls.data(); r.trim5 = trim5.data(); r.trim3 = trim3.data(); r.poly_len = poly.data(); r.dust = dust.data();
        r.seqs = seqs.data(); r.quals = quals.data(); r.offsets = offsets.data();
        return &r;
    }
};
clean::Rule clean_rule(const mapad_clean_params_t& p) {
    return clean::Rule{p.ops, p.poly_base, p.poly_min_len, p.poly_one_in, p.poly_max_mismatch, p.min_quality, p.min_length, p.max_dust};
}
bool clean_dust_counted(const clean::Rule& R, uint32_t cls) {
    return (R.ops & clean::OP_DUST) && (cls == clean::CLS_KEPT || cls == clean::CLS_TRIMMED || cls == clean::CLS_LOW_COMPLEXITY);
}
}  // namespace

struct mapad_cleaner {
    int device = 0;
    mapad_clean_params_t params{};
    clean::Rule rule{};
    hipStream_t own = nullptr;     // non-blocking, created with the cleaner
    hipStream_t stream = nullptr;  // `own`, or the caller's (mapad_cleaner_set_stream)
    DevBuf<uint8_t> d_seqs, d_quals, d_cls, d_out_seqs, d_out_quals;
    DevBuf<uint64_t> d_offs, d_out_offs;
    DevBuf<uint16_t> d_trim5, d_trim3, d_poly, d_dust;
    DevBuf<uint32_t> d_len;
    DevBuf<unsigned long long> d_tiles, d_counters;
    DevEvent ev[4];
    mapad_clean_counts_t totals{};
};

namespace {
// decide, scan, (wait for the total), write: everything on c->stream; the inputs are device pointers.  `counts` gets this call's counters (the call waits for them)
int clean_run_device(mapad_cleaner* c, const uint8_t* s, const uint8_t* q, const uint64_t* o, uint64_t n, uint64_t& total, mapad_clean_counts_t& counts, float ms[2]) {
    int rc;
    hipStream_t st = c->stream;
    const uint64_t n_tiles = (n + kScanTile - 1) / kScanTile;
    if ((rc = c->d_cls.ensure(n)) || (rc = c->d_trim5.ensure(n)) || (rc = c->d_trim3.ensure(n)) || (rc = c->d_poly.ensure(n)) || (rc = c->d_dust.ensure(n)) ||
        (rc = c->d_len.ensure(n)) || (rc = c->d_out_offs.ensure(n + 1)) || (rc = c->d_tiles.ensure(n_tiles + 1)) || (rc = c->d_counters.ensure(kCleanCounters, true))) return rc;
    for (auto& e : c->ev) if ((rc = e.ensure())) return rc;
    CleanDev Q{};
    Q.R = c->rule;
    Q.seqs = s; Q.quals = q; Q.offs = o; Q.n_reads = n;
    Q.cls = c->d_cls.p; Q.trim5 = c->d_trim5.p; Q.trim3 = c->d_trim3.p; Q.poly = c->d_poly.p; Q.dust = c->d_dust.p; Q.out_len = c->d_len.p; Q.out_offs = c->d_out_offs.p;
    Q.counters = c->d_counters.p;
    MergeDev S{};  // what the merge stage's scan launches read and write: the lengths, the tile sums, the offsets
    S.n_pairs = n; S.out_len = c->d_len.p; S.out_offs = c->d_out_offs.p; S.tile_sums = c->d_tiles.p;
    if ((rc = zero_async(st, Q.counters, kCleanCounters * sizeof(unsigned long long)))) return rc;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kCleanBlock / 64 - 1) / (kCleanBlock / 64), 1u << 16);
    const uint32_t grid_write = std::min<uint32_t>(grid, 2048u);  // as the merge write kernel's: a few thousand end-of-block flushes whatever the batch
    HIP_TRY(hipEventRecord(c->ev[0], st));
    if (n) {
        hipLaunchKernelGGL(clean_decide_kernel, dim3(grid), dim3(kCleanBlock), 0, st, Q);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c->ev[1], st));
    if (n) hipLaunchKernelGGL(merge_sums_kernel, dim3((uint32_t)n_tiles), dim3(64), 0, st, S);
    hipLaunchKernelGGL(merge_scan_tiles_kernel, dim3(1), dim3(64), 0, st, S, n_tiles);
    if (n) hipLaunchKernelGGL(merge_offsets_kernel, dim3((uint32_t)n_tiles), dim3(64), 0, st, S);
    HIP_TRY(hipGetLastError());
    total = 0;
    HIP_TRY(hipMemcpyAsync(&total, S.out_offs + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = c->d_out_seqs.ensure(total)) || (rc = c->d_out_quals.ensure(total))) return rc;
    Q.out_seqs = c->d_out_seqs.p; Q.out_quals = c->d_out_quals.p;
    HIP_TRY(hipEventRecord(c->ev[2], st));
    if (n) {
        hipLaunchKernelGGL(clean_write_kernel, dim3(grid_write), dim3(kCleanBlock), 0, st, Q);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c->ev[3], st));
    std::vector<unsigned long long> h(kCleanCounters);
    HIP_TRY(hipMemcpyAsync(h.data(), Q.counters, kCleanCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&ms[0], c->ev[0], c->ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms[1], c->ev[2], c->ev[3]));
    counts = mapad_clean_counts_t{};
    counts.reads_seen = n; counts.calls = 1;
    for (uint32_t k = 0; k < clean::N_CLASSES; ++k) counts.class_counts[k] = h[k];
    counts.bases_in = h[kCleanBasesIn]; counts.bases_out = h[kCleanBasesOut]; counts.bases_poly = h[kCleanPoly]; counts.bases_trim5 = h[kCleanTrim5]; counts.bases_trim3 = h[kCleanTrim3];
    for (int k = 0; k < MAPAD_CLEAN_LEN_BINS; ++k) counts.length_histogram[k] = h[kCleanLenHist + k];
    for (int k = 0; k < MAPAD_CLEAN_DUST_BINS; ++k) counts.dust_histogram[k] = h[kCleanDustHist + k];
    mapad_clean_counts_add(&c->totals, &counts);
    return MAPAD_OK;
}
// uploads, the five launches, the copies back into `o`; returns with the stream drained on success.  On an error return work may still be queued: the caller waits
int clean_from_host_queued(mapad_cleaner* c, CleanResultOwner* o, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offs, uint64_t n) {
    int rc;
    hipStream_t st = c->stream;
    static const uint64_t zero = 0;
    const uint64_t b = n ? offs[n] : 0;
    if ((rc = merge_upload(st, c->d_seqs, seqs, b)) || (rc = merge_upload(st, c->d_quals, quals, b)) || (rc = merge_upload(st, c->d_offs, n ? offs : &zero, n + 1))) return rc;
    uint64_t total = 0;
    if ((rc = clean_run_device(c, c->d_seqs.p, c->d_quals.p, c->d_offs.p, n, total, o->r.counts, o->r.kernel_ms))) return rc;
    o->room(n);
    o->seqs.resize(total); o->quals.resize(total);
    if (n) {
        HIP_TRY(hipMemcpyAsync(o->cls.data(), c->d_cls.p, n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(o->trim5.data(), c->d_trim5.p, n * 2, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(o->trim3.data(), c->d_trim3.p, n * 2, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(o->poly.data(), c->d_poly.p, n * 2, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(o->dust.data(), c->d_dust.p, n * 2, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(o->offsets.data(), c->d_out_offs.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (total) {
        HIP_TRY(hipMemcpyAsync(o->seqs.data(), c->d_out_seqs.p, total, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(o->quals.data(), c->d_out_quals.p, total, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MAPAD_OK;
}
}  // namespace

extern "C" {
void mapad_clean_params_default(mapad_clean_params_t* out) {
    if (!out) return;
    *out = mapad_clean_params_t{};
    out->poly_base = 'G'; out->poly_min_len = 10; out->poly_one_in = 8; out->poly_max_mismatch = 5; out->min_quality = 2; out->min_length = 15; out->max_dust = 1000;
}
int mapad_clean_params_check(const mapad_clean_params_t* p) {
    if (!p) return MAPAD_ERR_INVALID;
    if (p->poly_base > 255 || !clean::valid_base((uint8_t)p->poly_base)) return MAPAD_ERR_INVALID;
    if (p->poly_min_len < 1 || p->poly_one_in < 1 || p->min_quality > 93 || p->max_dust > 1000 || (p->ops & ~(uint32_t)clean::OP_ALL)) return MAPAD_ERR_INVALID;
    return MAPAD_OK;
}
int mapad_cleaner_create(int device_id, const mapad_clean_params_t* params, mapad_cleaner_t** out) {
    if (!params || !out) return MAPAD_ERR_INVALID;
    int rc;
    if ((rc = mapad_clean_params_check(params))) return rc;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device_id < 0 || device_id >= n_dev) {
        std::fprintf(stderr, "mapad_amd: no usable HIP device (mapad_clean_reads_host is the host path of this stage)\n");
        return MAPAD_ERR_NO_DEVICE;
    }
    if (hipSetDevice(device_id) != hipSuccess) return MAPAD_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return MAPAD_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::fprintf(stderr, "mapad_amd: device %d is %s, this library is built for gfx950 only\n", device_id, prop.gcnArchName);
        return MAPAD_ERR_NO_DEVICE;
    }
    auto c = std::make_unique<mapad_cleaner>();
    c->device = device_id; c->params = *params; c->rule = clean_rule(*params);
    HIP_TRY(hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking));
    c->stream = c->own;
    *out = c.release();
    return MAPAD_OK;
}
int mapad_cleaner_set_stream(mapad_cleaner_t* c, void* s) { if (!c) return MAPAD_ERR_INVALID; c->stream = s ? (hipStream_t)s : c->own; return MAPAD_OK; }
void mapad_cleaner_free(mapad_cleaner_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);  // the buffers free themselves on the cleaner's device
    if (c->own) { (void)hipStreamSynchronize(c->own); (void)hipStreamDestroy(c->own); }
    delete c;
}
int mapad_clean_reads(mapad_cleaner_t* c, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n, mapad_clean_result_t** out) {
    if (!c || !out) return MAPAD_ERR_INVALID;
    if (n && (!seqs || !quals || !offsets)) return MAPAD_ERR_INVALID;
    if (n >= 0xFFFFFFF0ull) return MAPAD_ERR_INVALID;
    if (hipSetDevice(c->device) != hipSuccess) return MAPAD_ERR_NO_DEVICE;
    try {
        auto o = std::make_unique<CleanResultOwner>();
        const int rc = clean_from_host_queued(c, o.get(), seqs, quals, offsets, n);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }  // nothing queued may still read the caller's arrays or write into `o` once this returns
        *out = o.release()->publish(n);
        return MAPAD_OK;
    } catch (const std::bad_alloc&) { (void)hipStreamSynchronize(c->stream); return MAPAD_ERR_NOMEM; }
}
void mapad_clean_result_free(mapad_clean_result_t* r) { delete reinterpret_cast<CleanResultOwner*>(r); }
void mapad_clean_counts_add(mapad_clean_counts_t* dst, const mapad_clean_counts_t* src) {
    if (!dst || !src) return;
    dst->reads_seen += src->reads_seen; dst->bases_in += src->bases_in; dst->bases_out += src->bases_out; dst->calls += src->calls;
    dst->bases_poly += src->bases_poly; dst->bases_trim5 += src->bases_trim5; dst->bases_trim3 += src->bases_trim3;
    for (int k = 0; k < MAPAD_CLEAN_CLASSES; ++k) dst->class_counts[k] += src->class_counts[k];
    for (int k = 0; k < MAPAD_CLEAN_LEN_BINS; ++k) dst->length_histogram[k] += src->length_histogram[k];
    for (int k = 0; k < MAPAD_CLEAN_DUST_BINS; ++k) dst->dust_histogram[k] += src->dust_histogram[k];
}
int mapad_cleaner_totals(mapad_cleaner_t* c, mapad_clean_counts_t* out) { if (!c || !out) return MAPAD_ERR_INVALID; *out = c->totals; return MAPAD_OK; }
int mapad_cleaner_reset(mapad_cleaner_t* c) { if (!c) return MAPAD_ERR_INVALID; c->totals = mapad_clean_counts_t{}; return MAPAD_OK; }
int mapad_clean_reads_device(mapad_cleaner_t* c, const void* d_seqs, const void* d_quals, const void* d_offsets, uint64_t n, void** d_out_seqs, void** d_out_quals,
                             void** d_out_offsets, uint64_t* total_bases) {
    if (!c || !d_out_seqs || !d_out_quals || !d_out_offsets || !total_bases) return MAPAD_ERR_INVALID;
    if (n && (!d_seqs || !d_quals || !d_offsets)) return MAPAD_ERR_INVALID;
    if (n >= 0xFFFFFFF0ull) return MAPAD_ERR_INVALID;
    if (hipSetDevice(c->device) != hipSuccess) return MAPAD_ERR_NO_DEVICE;
    try {
        auto counts = std::make_unique<mapad_clean_counts_t>();
        float ms[2];
        const int rc = clean_run_device(c, (const uint8_t*)d_seqs, (const uint8_t*)d_quals, (const uint64_t*)d_offsets, n, *total_bases, *counts, ms);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }  // nothing queued may still read the caller's buffers
        *d_out_seqs = c->d_out_seqs.p; *d_out_quals = c->d_out_quals.p; *d_out_offsets = c->d_out_offs.p;
        return MAPAD_OK;
    } catch (const std::bad_alloc&) { (void)hipStreamSynchronize(c->stream); return MAPAD_ERR_NOMEM; }
}
int mapad_clean_reads_host(const mapad_clean_params_t* params, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offs, uint64_t n, mapad_clean_result_t** out) {
    if (!params || !out || mapad_clean_params_check(params)) return MAPAD_ERR_INVALID;
    if (n && (!seqs || !quals || !offs)) return MAPAD_ERR_INVALID;
    try {
        const clean::Rule R = clean_rule(*params);
        auto o = std::make_unique<CleanResultOwner>();
        o->room(n);
        std::vector<uint32_t> len(n), src(n);
        merge_threads(n, [&](uint64_t lo, uint64_t hi, unsigned) {
            for (uint64_t r = lo; r < hi; ++r) {
                const clean::Decision D = clean::decide(R, seqs + offs[r], quals + offs[r], offs[r + 1] - offs[r]);
                o->cls[r] = (uint8_t)D.cls; o->trim5[r] = (uint16_t)D.trim5; o->trim3[r] = (uint16_t)D.trim3; o->poly[r] = (uint16_t)D.poly_len; o->dust[r] = (uint16_t)D.dust;
                len[r] = D.out_len; src[r] = D.src;
            }
        });
        o->offsets[0] = 0;
        for (uint64_t r = 0; r < n; ++r) o->offsets[r + 1] = o->offsets[r] + len[r];
        o->seqs.resize(o->offsets[n]); o->quals.resize(o->offsets[n]);
        std::mutex mu;
        mapad_clean_counts_t& total = o->r.counts;
        merge_threads(n, [&](uint64_t lo, uint64_t hi, unsigned) {
            auto c = std::make_unique<mapad_clean_counts_t>();
            for (uint64_t r = lo; r < hi; ++r) {
                if (len[r]) {
                    std::memcpy(o->seqs.data() + o->offsets[r], seqs + offs[r] + src[r], len[r]);
                    std::memcpy(o->quals.data() + o->offsets[r], quals + offs[r] + src[r], len[r]);
                }
                c->class_counts[o->cls[r]] += 1;
                c->bases_in += offs[r + 1] - offs[r]; c->bases_out += len[r];
                c->bases_poly += o->poly[r]; c->bases_trim5 += o->trim5[r]; c->bases_trim3 += (uint64_t)(o->trim3[r] - o->poly[r]);
                if (clean::yields_read(o->cls[r]) && len[r] < MAPAD_CLEAN_LEN_BINS) c->length_histogram[len[r]] += 1;
                if (clean_dust_counted(R, o->cls[r])) c->dust_histogram[o->dust[r] / 10] += 1;
            }
            c->reads_seen = hi - lo;
            std::lock_guard<std::mutex> g(mu);
            mapad_clean_counts_add(&total, c.get());
        });
        total.calls = 1;
        *out = o.release()->publish(n);
        return MAPAD_OK;
    } catch (const std::bad_alloc&) { return MAPAD_ERR_NOMEM; }
}
}  // extern "C"
