// k_clean.hpp — fragment of mapad_amd.hip (device half; not a stand-alone header): the clean_* kernels of the read clean-up (clean_core.hpp).  Relies on
// k_merge.hpp in front of it: the offsets are merge_sums_kernel + merge_scan_tiles_kernel + merge_offsets_kernel over a MergeDev that carries nothing but the
// lengths.  Launched from abi_clean.hpp.

namespace {

// ---- read clean-up (clean_core.hpp) -----------------------------------------------------------------------------------------------------------------------------
// In front of mapping and without an index: mapad_cleaner.  Per call
//   clean_decide_kernel   one wavefront per read: the poly tail, the two ends and the complexity windows in trips of 64 lanes, every decision from ballots (no LDS);
//   the merge stage's three scan launches: offsets = the exclusive prefix sum of the output lengths;
//   clean_write_kernel    one wavefront per read, lanes over the output columns; the counters and the two histograms.
struct CleanDev {
    clean::Rule R;
    const uint8_t* seqs; const uint8_t* quals; const uint64_t* offs;
    uint64_t n_reads;
    uint8_t* cls; uint16_t* trim5; uint16_t* trim3; uint16_t* poly; uint16_t* dust; uint32_t* out_len;  // [n_reads]
    const uint64_t* out_offs;                                                                           // [n_reads + 1]
    uint8_t* out_seqs; uint8_t* out_quals;
    unsigned long long* counters;  // [kCleanCounters]: the classes, bases in, out, poly, 5', 3', then the two histograms
};
constexpr uint32_t kCleanBlock = 256, kCleanBasesIn = clean::N_CLASSES, kCleanBasesOut = kCleanBasesIn + 1, kCleanPoly = kCleanBasesIn + 2, kCleanTrim5 = kCleanBasesIn + 3,
                   kCleanTrim3 = kCleanBasesIn + 4, kCleanLenHist = kCleanBasesIn + 5, kCleanDustHist = kCleanLenHist + clean::kLenBins;
constexpr uint32_t kCleanCounters = kCleanDustHist + clean::kDustBins;

__global__ void __launch_bounds__(kCleanBlock) clean_decide_kernel(CleanDev Q) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    constexpr uint32_t kWaves = kCleanBlock / 64;
    const clean::Rule& R = Q.R;
    for (uint64_t r = (uint64_t)blockIdx.x * kWaves + wave; r < Q.n_reads; r += (uint64_t)gridDim.x * kWaves) {  // (everything about r is uniform over the wavefront)
        const uint64_t o = Q.offs[r], len = Q.offs[r + 1] - o;
        uint32_t cls, t5 = 0, t3 = 0, poly = 0, dust = 0, out_len = 0;
        if (len == 0) cls = clean::CLS_EMPTY;
        else if (len > (uint64_t)clean::kMaxLen) { cls = clean::CLS_TOO_LONG; out_len = (uint32_t)(len < 0xFFFFFFFFull ? len : 0xFFFFFFFFull); }
        else {
            const uint32_t L = (uint32_t)len;
            const uint8_t* s = Q.seqs + o;
            const uint8_t* q = Q.quals + o;
            if (R.ops & clean::OP_POLY) {
                uint32_t carry = 0;
                for (uint32_t t = 0; 64u * t < L; ++t) {  // lane l: the n-th base from the 3' end
                    const uint32_t n = 64u * t + lane + 1u;
                    const bool in = n <= L;
                    const uint8_t b = in ? s[L - n] : (uint8_t)0;
                    const unsigned long long not_base = __ballot(in && b != (uint8_t)R.poly_base);
                    const uint32_t x = clean::poly_x(not_base, carry, lane);
                    const unsigned long long stop = __ballot(!in || clean::poly_stop(R, n, x)), cand = __ballot(in && clean::poly_candidate(R, n, b));
                    const uint32_t tail = clean::poly_trip_tail(stop, cand, t);
                    if (tail) poly = tail;
                    if (stop) break;
                    carry += (uint32_t)__popcll(not_base);
                }
            }
            const uint32_t E = L - poly;
            if (R.ops & (clean::OP_TRIM_N | clean::OP_TRIM_QUAL)) {
                for (uint32_t base = 0; base < E; base += 64u) {  // the 3' end first: lane l holds position E - 1 - (base + l); a lane past the 5' end ends the run
                    const uint32_t i = base + lane;
                    const bool in = i < E;
                    const uint32_t run = clean::run_length(__ballot(in && clean::removable(R, s[in ? E - 1u - i : 0u], q[in ? E - 1u - i : 0u])));
                    t3 += run;
                    if (run < 64u) break;
                }
                const uint32_t E5 = E - t3;
                for (uint32_t base = 0; base < E5; base += 64u) {
                    const uint32_t i = base + lane;
                    const bool in = i < E5;
                    const uint32_t run = clean::run_length(__ballot(in && clean::removable(R, s[in ? i : 0u], q[in ? i : 0u])));
                    t5 += run;
                    if (run < 64u) break;
                }
            }
            const uint32_t M = E - t3 - t5;
            if (M >= R.min_length && (R.ops & clean::OP_DUST)) {
                const uint8_t* w = s + t5;
                for (uint32_t k = 0;; ++k) {  // window k: lane l holds the base at 32 k + l and, from its two neighbours, the triplet that starts there
                    const uint32_t i = 32u * k + lane;
                    const uint32_t c0 = i < M ? (uint32_t)base_index(w[i]) : 4u;
                    const uint32_t c1 = (uint32_t)__shfl_down((int)c0, 1), c2 = (uint32_t)__shfl_down((int)c0, 2);  // (lanes 62 and 63 get their own value back and count nothing)
                    const bool counted = clean::dust_counted(lane, c0, c1, c2);
                    const uint32_t code = counted ? clean::dust_code(c0, c1, c2) : 0u;
                    const unsigned long long C = __ballot(counted);
                    uint64_t B[6];
#pragma unroll
                    for (int b = 0; b < 6; ++b) B[b] = __ballot(counted && ((code >> b) & 1u));
                    uint32_t S = counted ? clean::dust_lane_pairs(B, C, code, lane) : 0u;
                    for (int d = 32; d; d >>= 1) S += (uint32_t)__shfl_xor((int)S, d);
                    const uint32_t score = clean::dust_score(S, (uint32_t)__popcll(C));
                    dust = score > dust ? score : dust;
                    if (clean::dust_last_window(k, M)) break;
                }
            }
            t3 += poly;
            cls = clean::final_class(R, L, M, dust);
            if (clean::yields_read(cls)) out_len = M;
        }
        if (lane == 0) {
            Q.cls[r] = (uint8_t)cls; Q.trim5[r] = (uint16_t)t5; Q.trim3[r] = (uint16_t)t3; Q.poly[r] = (uint16_t)poly; Q.dust[r] = (uint16_t)dust; Q.out_len[r] = out_len;
        }
    }
}
__global__ void __launch_bounds__(kCleanBlock) clean_write_kernel(CleanDev Q) {
    constexpr uint32_t kBins = clean::kLenBins + clean::kDustBins;
    __shared__ uint32_t hist[kBins];  // the lengths, then the dust bins
    for (uint32_t i = threadIdx.x; i < kBins; i += kCleanBlock) hist[i] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    constexpr uint32_t kWaves = kCleanBlock / 64;
    uint32_t n_cls[clean::N_CLASSES] = {0, 0, 0, 0, 0, 0};  // lane 0's counts
    unsigned long long n_in = 0, n_out = 0, n_poly = 0, n_t5 = 0, n_t3 = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * kWaves + wave; r < Q.n_reads; r += (uint64_t)gridDim.x * kWaves) {
        const uint64_t o = Q.offs[r], out = Q.out_offs[r];
        const uint32_t cls = Q.cls[r], len = Q.out_len[r], t5 = Q.trim5[r];
        // (len > 0 only for a class that yields a read: t5 + len <= the read's length, and a too_long read has t5 == 0 and len == its length)
        const uint8_t* s = Q.seqs + o + t5;
        const uint8_t* q = Q.quals + o + t5;
        for (uint32_t p = lane; p < len; p += 64u) { Q.out_seqs[out + p] = s[p]; Q.out_quals[out + p] = q[p]; }
        if (lane == 0) {
#pragma unroll
            for (uint32_t k = 0; k < clean::N_CLASSES; ++k) n_cls[k] += cls == k;
            const uint32_t poly = Q.poly[r];
            n_in += Q.offs[r + 1] - o; n_out += len; n_poly += poly; n_t5 += t5; n_t3 += Q.trim3[r] - poly;
            if (clean::yields_read(cls) && len < (uint32_t)clean::kLenBins) atomicAdd(&hist[len], 1u);
            if ((Q.R.ops & clean::OP_DUST) && (cls == clean::CLS_KEPT || cls == clean::CLS_TRIMMED || cls == clean::CLS_LOW_COMPLEXITY))
                atomicAdd(&hist[clean::kLenBins + Q.dust[r] / 10u], 1u);  // dust <= 1000
        }
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < clean::N_CLASSES; ++k) if (n_cls[k]) atomicAdd(Q.counters + k, (unsigned long long)n_cls[k]);
        if (n_in) atomicAdd(Q.counters + kCleanBasesIn, n_in);
        if (n_out) atomicAdd(Q.counters + kCleanBasesOut, n_out);
        if (n_poly) atomicAdd(Q.counters + kCleanPoly, n_poly);
        if (n_t5) atomicAdd(Q.counters + kCleanTrim5, n_t5);
        if (n_t3) atomicAdd(Q.counters + kCleanTrim3, n_t3);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kBins; i += kCleanBlock) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(Q.counters + kCleanLenHist + i, (unsigned long long)v);  // (the dust bins lie right behind the length bins in both)
    }
}

}  // namespace
