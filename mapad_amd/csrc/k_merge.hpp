// k_merge.hpp — fragment of mapad_amd.hip (device half; not a stand-alone header): the merge_* kernels of adapter trimming and read-pair merging
// (merge_core.hpp).  Relies on what mapad_amd.hip defines in front of it: MAPAD_SLIM and kScanTile (the collect section).  Launched from abi_merge.hpp.

namespace {

// ---- adapter trimming and read-pair merging (merge_core.hpp) ---------------------------------------------------------------------
// In front of mapping and without an index: mapad_merger.  Per call
//   merge_decide_kernel   one wavefront per pair: the planes of X and Y into the wavefront's LDS, a candidate per lane, the winner by a wavefront-wide maximum;
//   merge_sums_kernel + merge_scan_tiles_kernel + merge_offsets_kernel: offsets = the exclusive prefix sum of the output lengths (the collect's scan reads hit
//                         pools, so this is its own: one length per pair);
//   merge_write_kernel    one wavefront per pair, lanes over the output columns; the counters and the length histogram.
struct MergeDev {
    merge::Rule R;
    const uint8_t* seqs1; const uint8_t* quals1; const uint64_t* offs1;
    const uint8_t* seqs2; const uint8_t* quals2; const uint64_t* offs2;  // single-end: nullptr
    uint64_t n_pairs;
    uint8_t* cls; int32_t* frag_len; uint16_t* m; uint16_t* x; uint32_t* out_len;  // [n_pairs]
    uint64_t* out_offs;                                                            // [n_pairs + 1]
    unsigned long long* tile_sums;                                                 // [n_tiles]
    uint8_t* out_seqs; uint8_t* out_quals;
    unsigned long long* counters;  // [kMergeCounters]: the classes, bases in, bases out, then the histogram
};
constexpr uint32_t kMergeBlock = 256, kMergeBasesIn = merge::N_CLASSES, kMergeBasesOut = merge::N_CLASSES + 1, kMergeHist = merge::N_CLASSES + 2;
constexpr uint32_t kMergeCounters = kMergeHist + merge::kHistBins;
// the lengths of pair r's mates, clamped so that they fit an int (anything above kMaxMate is too_long)
__device__ __forceinline__ void merge_lengths(const MergeDev& Q, uint64_t r, uint64_t& o1, uint64_t& o2, int& L1, int& L2) {
    o1 = Q.offs1[r]; o2 = 0; L2 = 0;
    const uint64_t l1 = Q.offs1[r + 1] - o1;
    L1 = (int)(l1 < 0x7FFFFFFFull ? l1 : 0x7FFFFFFFull);
    if (Q.R.mode == merge::MODE_PAIRS) {
        o2 = Q.offs2[r];
        const uint64_t l2 = Q.offs2[r + 1] - o2;
        L2 = (int)(l2 < 0x7FFFFFFFull ? l2 : 0x7FFFFFFFull);
    }
}
__global__ void __launch_bounds__(kMergeBlock) merge_decide_kernel(MergeDev Q) {
    __shared__ merge::Planes planes[kMergeBlock / 64][2];  // 432 B per wavefront
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    constexpr uint32_t kWaves = kMergeBlock / 64;
    merge::Planes& X = planes[wave][0];
    merge::Planes& Y = planes[wave][1];
    for (uint64_t r = (uint64_t)blockIdx.x * kWaves + wave; r < Q.n_pairs; r += (uint64_t)gridDim.x * kWaves) {  // (everything about r is uniform over the wavefront)
        uint64_t o1, o2;
        int L1, L2;
        merge_lengths(Q, r, o1, o2, L1, L2);
        uint32_t cls = merge::early_class(Q.R, L1, L2), key = 0, bm = 0, bx = 0;
        int out_len = 0;
        if (cls == merge::N_CLASSES) {
            const uint8_t* r1 = Q.seqs1 + o1;
            const uint8_t* r2 = Q.seqs2 + o2;  // not read while L2 == 0
            const int nx = (int)Q.R.a2_len + L1, ny = L2 + (int)Q.R.a1_len;
            for (int w = 0; w < merge::kPlaneWords; ++w) {
                const int i = 64 * w + (int)lane;
                const uint32_t cx = i < nx ? merge::code3(merge::x_byte(Q.R, r1, L1, i)) : 0u, cy = i < ny ? merge::code3(merge::y_byte(Q.R, r2, L2, i)) : 0u;
                const unsigned long long x0 = __ballot(cx & 1u), x1 = __ballot(cx & 2u), xv = __ballot(cx & 4u);
                const unsigned long long y0 = __ballot(cy & 1u), y1 = __ballot(cy & 2u), yv = __ballot(cy & 4u);
                if (lane == 0) { X.c0[w] = x0; X.c1[w] = x1; X.v[w] = xv; Y.c0[w] = y0; Y.c1[w] = y1; Y.v[w] = yv; }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the lanes read lane 0's words: LDS serves a wavefront's accesses in order, the compiler must keep them so
            __builtin_amdgcn_wave_barrier();
            const int fmax = merge::max_candidate(Q.R, L1, L2);
            for (int F = (int)lane; F <= fmax; F += 64) {  // a candidate per lane; no cross-lane operation in here
                int m, x;
                merge::candidate_counts(X, Y, Q.R, L1, L2, F, m, x);
                const uint32_t k = merge::order_key(Q.R, F, m, x);
                if (k > key) { key = k; bm = (uint32_t)m; bx = (uint32_t)x; }
            }
            uint32_t best = key;
            for (int d = 32; d; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)best, d); best = o > best ? o : best; }
            const unsigned long long owner = __ballot(best != 0u && key == best);  // one lane: admissible keys differ in F
            if (owner) {
                const int src = __ffsll((long long)owner) - 1;
                bm = (uint32_t)__shfl((int)bm, src); bx = (uint32_t)__shfl((int)bx, src);
            } else { bm = 0; bx = 0; }
            key = best;
            cls = merge::final_class(Q.R, L1, key, out_len);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the next pair's words go where these were read
            __builtin_amdgcn_wave_barrier();
        }
        if (lane == 0) {
            Q.cls[r] = (uint8_t)cls; Q.frag_len[r] = key ? merge::key_frag_len(key) : -1; Q.m[r] = (uint16_t)bm; Q.x[r] = (uint16_t)bx; Q.out_len[r] = (uint32_t)out_len;
        }
    }
}
__device__ __forceinline__ void wave_scan1(unsigned long long& a, uint32_t lane) {  // inclusive scan over the wavefront's lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long ua = __shfl_up(a, d);
        if (lane >= (uint32_t)d) a += ua;
    }
}
__global__ void MAPAD_SLIM merge_sums_kernel(MergeDev Q) {
    unsigned long long s = 0;
    for (int q = 0; q < 4; ++q) {
        const uint64_t r = (uint64_t)blockIdx.x * kScanTile + q * 64 + threadIdx.x;
        if (r < Q.n_pairs) s += Q.out_len[r];
    }
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
    if (threadIdx.x == 0) Q.tile_sums[blockIdx.x] = s;
}
__global__ void MAPAD_SLIM merge_scan_tiles_kernel(MergeDev Q, uint64_t n_tiles) {  // one wavefront: exclusive scan of the tile sums, the total behind the last pair
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n_tiles; base += 64) {
        const uint64_t i = base + lane;
        const unsigned long long v = i < n_tiles ? Q.tile_sums[i] : 0;
        unsigned long long s = v;
        wave_scan1(s, lane);
        if (i < n_tiles) Q.tile_sums[i] = carry + s - v;
        carry += __shfl(s, 63);
    }
    if (lane == 0) Q.out_offs[Q.n_pairs] = carry;
}
__global__ void MAPAD_SLIM merge_offsets_kernel(MergeDev Q) {  // tile-local exclusive scan: lane t owns pairs 4t .. 4t+3 of the tile
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r0 = (uint64_t)blockIdx.x * kScanTile + 4 * lane;
    uint32_t c[4];
    unsigned long long t = 0;
    for (int q = 0; q < 4; ++q) { c[q] = r0 + q < Q.n_pairs ? Q.out_len[r0 + q] : 0; t += c[q]; }
    unsigned long long s = t;
    wave_scan1(s, lane);
    unsigned long long b = Q.tile_sums[blockIdx.x] + s - t;
    for (int q = 0; q < 4; ++q) {
        if (r0 + q >= Q.n_pairs) break;
        Q.out_offs[r0 + q] = b;
        b += c[q];
    }
}
__global__ void __launch_bounds__(kMergeBlock) merge_write_kernel(MergeDev Q) {
    __shared__ uint32_t hist[merge::kHistBins];
    for (uint32_t i = threadIdx.x; i < (uint32_t)merge::kHistBins; i += kMergeBlock) hist[i] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    constexpr uint32_t kWaves = kMergeBlock / 64;
    uint32_t n_cls[merge::N_CLASSES] = {0, 0, 0, 0, 0};  // lane 0's counts
    unsigned long long n_in = 0, n_out = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * kWaves + wave; r < Q.n_pairs; r += (uint64_t)gridDim.x * kWaves) {
        uint64_t o1, o2;
        int L1, L2;
        merge_lengths(Q, r, o1, o2, L1, L2);
        const uint32_t cls = Q.cls[r];
        const int len = (int)Q.out_len[r], F = Q.R.mode == merge::MODE_SINGLE ? len : Q.frag_len[r];
        const uint64_t out = Q.out_offs[r];
        // (len > 0 only behind a compare: both mates are at most kMaxMate long, F <= L1 + L2, and every index column() forms lies inside its mate)
        for (int p = (int)lane; p < len; p += 64) {
            uint8_t b, q;
            merge::column(Q.R, Q.seqs1 + o1, Q.quals1 + o1, L1, Q.seqs2 + o2, Q.quals2 + o2, L2, F, p, b, q);
            Q.out_seqs[out + p] = b; Q.out_quals[out + p] = q;
        }
        if (lane == 0) {
#pragma unroll
            for (uint32_t k = 0; k < merge::N_CLASSES; ++k) n_cls[k] += cls == k;
            n_in += (uint64_t)(Q.offs1[r + 1] - o1) + (Q.R.mode == merge::MODE_PAIRS ? Q.offs2[r + 1] - o2 : 0ull);
            n_out += (unsigned long long)len;
            if (merge::yields_read(Q.R, cls) && len < merge::kHistBins) atomicAdd(&hist[len], 1u);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < merge::N_CLASSES; ++k) if (n_cls[k]) atomicAdd(Q.counters + k, (unsigned long long)n_cls[k]);
        if (n_in) atomicAdd(Q.counters + kMergeBasesIn, n_in);
        if (n_out) atomicAdd(Q.counters + kMergeBasesOut, n_out);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (uint32_t)merge::kHistBins; i += kMergeBlock) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(Q.counters + kMergeHist + i, (unsigned long long)v);
    }
}

}  // namespace
