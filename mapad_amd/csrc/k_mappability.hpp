// k_mappability.hpp — fragment of mapad_amd.hip (device half, last; not a stand-alone header): the mappability kernels, loci of every reference k-mer
// (mappability_core.hpp).  Relies on what mapad_amd.hip defines in front of it (MAPAD_SLIM); launched from abi_mappability.hpp.

namespace {

// ---- mappability: loci of every reference k-mer (mappability_core.hpp) -------------------------------------------------------------------------------
// A tile of starts of one contig.  The count kernel: one quad per start, sixteen starts per wavefront, four rounds per block; the block's bases are staged
// packed in LDS first.  Every branch and every loop of count_start is quad-uniform (the quad's intervals are), so the DPP moves of the rank queries always
// find their four lanes active.  Quads of a wavefront whose chains differ in length wait for each other: neighbouring starts mostly do not.
struct MappabilityDev {
    const uint8_t* seq;            // the caller's bases from the tile's first start on
    uint64_t avail;                // ... how many of them there are (the contig ends behind them)
    uint64_t n_starts;
    int k, e, full;
    uint8_t* counts;               // [n_starts]
    uint32_t* flag;                // raised when `full` and a valid start counts 0
    unsigned long long* steps;     // extension steps taken (null: not counted)
};
__global__ __launch_bounds__(mappability::kBlockStarts) void mappability_count_kernel(DevIndex ix, MappabilityDev q) {
    using namespace mappability;
    __shared__ uint32_t s_base[kStageWords];
    __shared__ uint16_t s_valid[kStageWords];
    __shared__ uint32_t s_steps;
    const uint64_t blk0 = (uint64_t)blockIdx.x * kBlockStarts;
    if (threadIdx.x < (uint32_t)kStageWords) {
        const uint64_t at = blk0 + 16ull * threadIdx.x;
        uint32_t b, v;
        pack16(q.seq + at, at < q.avail ? q.avail - at : 0, b, v);
        s_base[threadIdx.x] = b; s_valid[threadIdx.x] = (uint16_t)v;
    }
    if (threadIdx.x == 0) s_steps = 0;
    __syncthreads();
    const Staged st{s_base, s_valid};
    const QuadQuery query{(int)(threadIdx.x & 3u)};
    const int quad = (int)(threadIdx.x >> 2);
    uint32_t steps = 0;
    for (int round = 0; round < 4; ++round) {
        const int p = quad + 64 * round;
        if (blk0 + (uint64_t)p >= q.n_starts) break;
        uint32_t c = 0;
        if (staged_valid(st, p, q.k)) {
            c = count_start(ix, st, p, q.k, q.e, q.full != 0, query, steps);
            if (q.full && c == 0) *q.flag = 1u;
        }
        if (query.w == 0) q.counts[blk0 + (uint64_t)p] = (uint8_t)c;
    }
    if (q.steps) {
        if (query.w == 0 && steps) atomicAdd(&s_steps, steps);
        __syncthreads();
        if (threadIdx.x == 0 && s_steps) atomicAdd(q.steps, (unsigned long long)s_steps);
    }
}

// cover(x) = starts s in [x - k + 1, x] with c(s) == 1, for the tile's positions: the flags of a block's starts and of the k - 1 before them as bits in LDS,
// a windowed popcount per position.  Starts in front of the tile come from halo_prev (the counts of the k - 1 starts before it; zero in front of the first
// tile); the last k - 1 counts up to the tile's end go to halo_next for the tile behind (the tile may be shorter than k - 1: then some come from halo_prev).
struct MappabilityCoverDev {
    const uint8_t* counts;
    const uint8_t* halo_prev;
    uint8_t* halo_next;
    uint8_t* cover;
    uint64_t n;
    int k;
};
__global__ __launch_bounds__(256) void mappability_cover_kernel(MappabilityCoverDev q) {
    __shared__ uint64_t s_bits[8];
    const long long h = q.k - 1, n = (long long)q.n;
    const long long blk0 = (long long)blockIdx.x * 256;
    for (int r = 0; r < 2; ++r) {
        const long long s = blk0 - h + (long long)threadIdx.x + 256 * r;  // start of staged bit threadIdx.x + 256 r
        bool one = false;
        if (s < blk0 + 256) {
            if (s >= 0) { if (s < n) one = q.counts[s] == 1; }
            else one = q.halo_prev[h + s] == 1;  // s >= -h
        }
        const unsigned long long b = __ballot(one);
        if ((threadIdx.x & 63u) == 0) s_bits[(threadIdx.x >> 6) + 4 * r] = b;
    }
    __syncthreads();
    const long long x = blk0 + threadIdx.x;
    if (x < n) q.cover[x] = (uint8_t)mappability::bits_in_range(s_bits, (int)threadIdx.x, q.k);
    if (x < h) {
        const long long s = n - h + x;
        q.halo_next[x] = s >= 0 ? q.counts[s] : q.halo_prev[h + s];
    }
}

// the figures of a tile into its contig's words and the total's (mappability::SUM_*)
struct MappabilitySumDev {
    const uint8_t* counts;
    const uint8_t* cover;
    uint64_t n, x0, len;           // x0: the contig position of the tile's first start
    uint32_t k;
    unsigned long long* contig;
    unsigned long long* total;
};
__global__ __launch_bounds__(256) void mappability_summary_kernel(MappabilitySumDev q) {
    using namespace mappability;
    __shared__ uint32_t s_sum[SUM_WORDS];
    if (threadIdx.x < (uint32_t)SUM_WORDS) s_sum[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < q.n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t c = q.counts[i], cov = q.cover[i], possible = possible_starts(q.x0 + i, q.k, q.len);
        if (c) { atomicAdd(&s_sum[SUM_VALID], 1u); atomicAdd(&s_sum[SUM_HIST + hist_bin(c)], 1u); }
        if (c == 1) atomicAdd(&s_sum[SUM_UNIQUE], 1u);
        if (mask_majority(cov, possible)) atomicAdd(&s_sum[SUM_MAJORITY], 1u);
        if (mask_strict(cov, possible)) atomicAdd(&s_sum[SUM_STRICT], 1u);
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)SUM_WORDS && s_sum[threadIdx.x]) {
        atomicAdd(q.contig + threadIdx.x, (unsigned long long)s_sum[threadIdx.x]);
        atomicAdd(q.total + threadIdx.x, (unsigned long long)s_sum[threadIdx.x]);
    }
}

}  // namespace
