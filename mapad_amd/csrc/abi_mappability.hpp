// abi_mappability.hpp — fragment of mapad_amd.hip (host half, last; not a stand-alone header): the mappability track on the device and on the host, and its
// ABI.  Relies on k_mappability.hpp, on lib_buffers.hpp (HIP_TRY) and on mapad_ctx in mapad_amd.hip (its mp_* members, stream and index).

// ---- mappability ---------------------------------------------------------------------------------------------------------------------------------------
namespace {
// starts per tile of the device path: the default, or what MAPAD_MAPPABILITY_TILE lowers it to (a test hook, read per call)
int mappability_tile(uint64_t& tile) {
    tile = mappability::kDefaultTile;
    const char* e = std::getenv("MAPAD_MAPPABILITY_TILE");
    if (!e || !*e) return MAPAD_OK;
    char* end = nullptr;
    const unsigned long long v = std::strtoull(e, &end, 10);
    if (e[0] < '0' || e[0] > '9' || *end || v == 0 || v > mappability::kDefaultTile) {
        std::fprintf(stderr, "mapad_amd: MAPAD_MAPPABILITY_TILE must be in [1, %u]\n", mappability::kDefaultTile);
        return MAPAD_ERR_PARSE;
    }
    tile = v;
    return MAPAD_OK;
}
int mappability_check(const host::Index& ix, uint32_t tid, const uint8_t* seq, uint64_t len, uint64_t from, uint64_t n, uint32_t k, uint32_t e, uint32_t flags) {
    if (k < 1 || k > (uint32_t)mappability::kMaxK || e > 1 || (flags & ~(uint32_t)MAPAD_MAPPABILITY_VERIFY)) return MAPAD_ERR_INVALID;
    if (tid >= ix.contigs.size()) return MAPAD_ERR_INVALID;
    if (len != ix.contigs[tid].end - ix.contigs[tid].start + 1 || (len && !seq)) return MAPAD_ERR_INVALID;
    if (from > len || n > len - from) return MAPAD_ERR_INVALID;
    return MAPAD_OK;
}
// the first start whose count a cover of [from, ..) needs
uint64_t mappability_halo_from(uint64_t from, uint32_t k) { return from >= k - 1 ? from - (k - 1) : 0; }

// Starts [from, from + n) of one contig on the device, tile by tile on the context's stream; waits for each tile.  out_counts / out_cover: host memory or null;
// d_contig / d_total: the summary's device words or null (then from == 0).  Adds to the context's mp_* figures.
int mappability_device(mapad_ctx* c, const uint8_t* seq, uint64_t len, uint64_t from, uint64_t n, uint32_t k, uint32_t e, bool full, uint8_t* out_counts,
                       uint8_t* out_cover, unsigned long long* d_contig, unsigned long long* d_total) {
    using namespace mappability;
    uint64_t tile;
    int rc;
    if ((rc = mappability_tile(tile))) return rc;
    if (n == 0) return MAPAD_OK;
    const bool want_cover = out_cover || d_contig;
    const uint64_t h = k - 1, first = want_cover ? mappability_halo_from(from, k) : from, end = from + n;
    tile = std::min<uint64_t>(tile, end - first);
    if ((rc = c->d_mp_seq.ensure(tile + kMaxK + 16))) return rc;
    if ((rc = c->d_mp_counts.ensure(tile))) return rc;
    if ((rc = c->d_mp_cover.ensure(tile))) return rc;
    if ((rc = c->d_mp_halo.ensure(512, true))) return rc;
    if ((rc = c->d_mp_sum.ensure(2, true))) return rc;
    for (auto& ev : c->ev_mp) if ((rc = ev.ensure())) return rc;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemsetAsync(c->d_mp_sum.p, 0, 2 * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(c->d_mp_halo.p, 0, 512, st));
    int cur = 0;
    for (uint64_t t0 = first; t0 < end; t0 += tile, cur ^= 1) {
        const uint64_t tn = std::min<uint64_t>(tile, end - t0), avail = std::min<uint64_t>(len, t0 + tn + h) - t0;
        HIP_TRY(hipMemcpyAsync(c->d_mp_seq.p, seq + t0, avail, hipMemcpyHostToDevice, st));
        MappabilityDev q{};
        q.seq = c->d_mp_seq.p; q.avail = avail; q.n_starts = tn; q.k = (int)k; q.e = (int)e; q.full = full ? 1 : 0;
        q.counts = c->d_mp_counts.p; q.steps = c->d_mp_sum.p; q.flag = reinterpret_cast<uint32_t*>(c->d_mp_sum.p + 1);
        HIP_TRY(hipEventRecord(c->ev_mp[0], st));
        hipLaunchKernelGGL(mappability_count_kernel, dim3((uint32_t)((tn + kBlockStarts - 1) / kBlockStarts)), dim3(kBlockStarts), 0, st, c->dix, q);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev_mp[1], st));
        if (want_cover) {
            MappabilityCoverDev v{c->d_mp_counts.p, c->d_mp_halo.p + 256 * cur, c->d_mp_halo.p + 256 * (cur ^ 1), c->d_mp_cover.p, tn, (int)k};
            hipLaunchKernelGGL(mappability_cover_kernel, dim3((uint32_t)((std::max(tn, h) + 255) / 256)), dim3(256), 0, st, v);
            HIP_TRY(hipGetLastError());
        }
        if (d_contig) {
            MappabilitySumDev s{c->d_mp_counts.p, c->d_mp_cover.p, tn, t0, len, k, d_contig, d_total};
            hipLaunchKernelGGL(mappability_summary_kernel, dim3((uint32_t)std::min<uint64_t>((tn + 255) / 256, 2048)), dim3(256), 0, st, s);
            HIP_TRY(hipGetLastError());
        }
        const uint64_t lo = std::max(t0, from);
        if (lo < t0 + tn) {
            if (out_counts) HIP_TRY(hipMemcpyAsync(out_counts + (lo - from), c->d_mp_counts.p + (lo - t0), t0 + tn - lo, hipMemcpyDeviceToHost, st));
            if (out_cover) HIP_TRY(hipMemcpyAsync(out_cover + (lo - from), c->d_mp_cover.p + (lo - t0), t0 + tn - lo, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_mp[0], c->ev_mp[1]));
        c->mp_kernel_ms += ms;
    }
    unsigned long long words[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(words, c->d_mp_sum.p, sizeof words, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->mp_starts += end - first; c->mp_steps += words[0];
    return full && (words[1] & 0xFFFFFFFFull) ? MAPAD_ERR_INVALID : MAPAD_OK;
}

// ... and on the host: the same count_start over host threads, a block of starts at a time; counts[i] is start first + i.  false: `full` and a valid start counts 0
bool mappability_host_counts(const host::Index& ix, const uint8_t* seq, uint64_t len, uint64_t first, uint64_t n, uint32_t k, uint32_t e, bool full, uint8_t* counts,
                             uint64_t& steps_out) {
    using namespace mappability;
    const DevIndex v = ix.view();
    const uint64_t n_blocks = (n + kBlockStarts - 1) / kBlockStarts;
    std::atomic<uint64_t> next{0}, steps{0};
    std::atomic<bool> bad{false};
    auto work = [&] {
        uint32_t base[kStageWords];
        uint16_t valid[kStageWords];
        uint64_t my_steps = 0;
        for (uint64_t b = next.fetch_add(1); b < n_blocks; b = next.fetch_add(1)) {
            const uint64_t blk0 = first + b * kBlockStarts;
            for (int w = 0; w < kStageWords; ++w) {
                const uint64_t at = blk0 + 16ull * w;
                uint32_t pb, pv;
                pack16(seq + at, at < len ? len - at : 0, pb, pv);
                base[w] = pb; valid[w] = (uint16_t)pv;
            }
            const Staged st{base, valid};
            const int in_block = (int)std::min<uint64_t>(kBlockStarts, first + n - blk0);
            for (int p = 0; p < in_block; ++p) {
                uint32_t c = 0, s = 0;
                if (staged_valid(st, p, (int)k)) {
                    c = count_start(v, st, p, (int)k, (int)e, full, ScalarQuery{}, s);
                    if (full && c == 0) bad = true;
                }
                counts[blk0 - first + p] = (uint8_t)c;
                my_steps += s;
            }
        }
        steps += my_steps;
    };
    const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(host::cpu_share(), n_blocks));
    if (T <= 1) work();
    else { std::vector<std::thread> pool; for (unsigned t = 0; t < T; ++t) pool.emplace_back(work); for (auto& th : pool) th.join(); }
    steps_out += steps.load();
    return !bad.load();
}
// cover of the positions first + i, i < n, from the counts of the same starts (a position's window is cut at `first`: see mappability_halo_from)
void mappability_host_cover(const uint8_t* counts, uint64_t n, uint32_t k, uint8_t* cover) {
    uint32_t run = 0;
    for (uint64_t i = 0; i < n; ++i) {
        run += counts[i] == 1;
        if (i >= k) run -= counts[i - k] == 1;
        cover[i] = (uint8_t)run;
    }
}
void mappability_host_sums(const uint8_t* counts, const uint8_t* cover, uint64_t len, uint32_t k, unsigned long long* sums) {
    using namespace mappability;
    for (uint64_t x = 0; x < len; ++x) {
        const uint32_t c = counts[x], possible = possible_starts(x, k, len);
        if (c) { ++sums[SUM_VALID]; ++sums[SUM_HIST + hist_bin(c)]; }
        if (c == 1) ++sums[SUM_UNIQUE];
        if (mask_majority(cover[x], possible)) ++sums[SUM_MAJORITY];
        if (mask_strict(cover[x], possible)) ++sums[SUM_STRICT];
    }
}
void mappability_fill(const unsigned long long* sums, uint64_t length, mapad_mappability_contig_t& o) {
    using namespace mappability;
    o.length = length; o.valid_starts = sums[SUM_VALID]; o.unique_starts = sums[SUM_UNIQUE];
    for (int b = 0; b < kBins; ++b) o.hist[b] = sums[SUM_HIST + b];
    o.majority = sums[SUM_MAJORITY]; o.strict = sums[SUM_STRICT];
}
int mappability_summary_check(const host::Index& ix, const uint8_t* const* seqs, const uint64_t* lens, uint32_t k, uint32_t e, uint32_t flags, const mapad_mappability_t* out) {
    if (!out || (ix.contigs.size() && (!seqs || !lens || !out->contigs)) || out->n_contigs < ix.contigs.size()) return MAPAD_ERR_INVALID;
    for (size_t i = 0; i < ix.contigs.size(); ++i) {
        const int rc = mappability_check(ix, (uint32_t)i, seqs[i], lens[i], 0, lens[i], k, e, flags);
        if (rc) return rc;
    }
    return k < 1 || k > (uint32_t)mappability::kMaxK || e > 1 || (flags & ~(uint32_t)MAPAD_MAPPABILITY_VERIFY) ? MAPAD_ERR_INVALID : MAPAD_OK;
}
void mappability_summary_out(const host::Index& ix, const std::vector<unsigned long long>& sums, uint32_t k, uint32_t e, uint64_t starts, uint64_t steps, double ms,
                             mapad_mappability_t* out) {
    const size_t nc = ix.contigs.size();
    uint64_t total_len = 0;
    for (size_t i = 0; i < nc; ++i) {
        const uint64_t len = ix.contigs[i].end - ix.contigs[i].start + 1;
        mappability_fill(sums.data() + mappability::SUM_WORDS * i, len, out->contigs[i]);
        total_len += len;
    }
    mappability_fill(sums.data() + mappability::SUM_WORDS * nc, total_len, out->total);
    out->n_contigs = (uint32_t)nc; out->k = k; out->e = e; out->pad = 0;
    out->starts = starts; out->steps = steps; out->kernel_ms = ms;
}
}  // namespace

extern "C" {
int mapad_ctx_mappability(mapad_ctx_t* ctx, uint32_t tid, const uint8_t* seq, uint64_t len, uint64_t from, uint64_t n, uint32_t k, uint32_t e, uint32_t flags,
                          uint8_t* out_counts, uint8_t* out_cover) {
    if (!ctx) return MAPAD_ERR_INVALID;
    int rc;
    if ((rc = mappability_check(ctx->index->ix, tid, seq, len, from, n, k, e, flags))) return rc;
    if (hipSetDevice(ctx->device) != hipSuccess) return MAPAD_ERR_NO_DEVICE;
    ctx->mp_kernel_ms = 0; ctx->mp_starts = 0; ctx->mp_steps = 0;
    return mappability_device(ctx, seq, len, from, n, k, e, (flags & MAPAD_MAPPABILITY_VERIFY) != 0, out_counts, out_cover, nullptr, nullptr);
}
int mapad_ctx_mappability_summary(mapad_ctx_t* ctx, const uint8_t* const* seqs, const uint64_t* lens, uint32_t k, uint32_t e, uint32_t flags, mapad_mappability_t* out) {
    if (!ctx) return MAPAD_ERR_INVALID;
    const host::Index& ix = ctx->index->ix;
    int rc;
    if ((rc = mappability_summary_check(ix, seqs, lens, k, e, flags, out))) return rc;
    if (hipSetDevice(ctx->device) != hipSuccess) return MAPAD_ERR_NO_DEVICE;
    try {
        const size_t nc = ix.contigs.size(), words = mappability::SUM_WORDS * (nc + 1);
        if ((rc = ctx->d_mp_sum.ensure(2 + words, true))) return rc;
        HIP_TRY(hipMemsetAsync(ctx->d_mp_sum.p, 0, (2 + words) * sizeof(unsigned long long), ctx->stream));
        ctx->mp_kernel_ms = 0; ctx->mp_starts = 0; ctx->mp_steps = 0;
        unsigned long long* d_sums = ctx->d_mp_sum.p + 2;
        for (size_t i = 0; i < nc; ++i)
            if ((rc = mappability_device(ctx, seqs[i], lens[i], 0, lens[i], k, e, (flags & MAPAD_MAPPABILITY_VERIFY) != 0, nullptr, nullptr,
                                         d_sums + mappability::SUM_WORDS * i, d_sums + mappability::SUM_WORDS * nc)))
                return rc;
        std::vector<unsigned long long> sums(words);
        HIP_TRY(hipMemcpyAsync(sums.data(), d_sums, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        mappability_summary_out(ix, sums, k, e, ctx->mp_starts, ctx->mp_steps, ctx->mp_kernel_ms, out);
        return MAPAD_OK;
    } catch (const std::bad_alloc&) { return MAPAD_ERR_NOMEM; }
}
int mapad_last_mappability_info(mapad_ctx_t* ctx, double* kernel_ms, uint64_t* starts, uint64_t* steps) {
    if (!ctx || !kernel_ms || !starts || !steps) return MAPAD_ERR_INVALID;
    *kernel_ms = ctx->mp_kernel_ms; *starts = ctx->mp_starts; *steps = ctx->mp_steps;
    return MAPAD_OK;
}
int mapad_mappability_host(const mapad_index_t* idx, uint32_t tid, const uint8_t* seq, uint64_t len, uint64_t from, uint64_t n, uint32_t k, uint32_t e, uint32_t flags,
                           uint8_t* out_counts, uint8_t* out_cover) {
    if (!idx) return MAPAD_ERR_INVALID;
    int rc;
    if ((rc = mappability_check(idx->ix, tid, seq, len, from, n, k, e, flags))) return rc;
    if (n == 0) return MAPAD_OK;
    try {
        const uint64_t first = out_cover ? mappability_halo_from(from, k) : from, m = from + n - first;
        std::vector<uint8_t> counts(m);
        uint64_t steps = 0;
        if (!mappability_host_counts(idx->ix, seq, len, first, m, k, e, (flags & MAPAD_MAPPABILITY_VERIFY) != 0, counts.data(), steps)) return MAPAD_ERR_INVALID;
        if (out_counts) std::memcpy(out_counts, counts.data() + (from - first), n);
        if (out_cover) {
            std::vector<uint8_t> cover(m);
            mappability_host_cover(counts.data(), m, k, cover.data());
            std::memcpy(out_cover, cover.data() + (from - first), n);
        }
        return MAPAD_OK;
    } catch (const std::bad_alloc&) { return MAPAD_ERR_NOMEM; }
}
int mapad_mappability_summary_host(const mapad_index_t* idx, const uint8_t* const* seqs, const uint64_t* lens, uint32_t k, uint32_t e, uint32_t flags,
                                   mapad_mappability_t* out) {
    if (!idx) return MAPAD_ERR_INVALID;
    const host::Index& ix = idx->ix;
    int rc;
    if ((rc = mappability_summary_check(ix, seqs, lens, k, e, flags, out))) return rc;
    try {
        const size_t nc = ix.contigs.size();
        std::vector<unsigned long long> sums(mappability::SUM_WORDS * (nc + 1), 0ull);
        uint64_t starts = 0, steps = 0;
        for (size_t i = 0; i < nc; ++i) {
            std::vector<uint8_t> counts(lens[i]), cover(lens[i]);
            if (!mappability_host_counts(ix, seqs[i], lens[i], 0, lens[i], k, e, (flags & MAPAD_MAPPABILITY_VERIFY) != 0, counts.data(), steps)) return MAPAD_ERR_INVALID;
            mappability_host_cover(counts.data(), lens[i], k, cover.data());
            mappability_host_sums(counts.data(), cover.data(), lens[i], k, sums.data() + mappability::SUM_WORDS * i);
            starts += lens[i];
        }
        for (size_t i = 0; i < nc; ++i)
            for (int w = 0; w < mappability::SUM_WORDS; ++w) sums[mappability::SUM_WORDS * nc + w] += sums[mappability::SUM_WORDS * i + w];
        mappability_summary_out(ix, sums, k, e, starts, steps, 0.0, out);
        return MAPAD_OK;
    } catch (const std::bad_alloc&) { return MAPAD_ERR_NOMEM; }
}
}  // extern "C"
