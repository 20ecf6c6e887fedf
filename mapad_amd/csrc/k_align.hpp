// k_align.hpp — fragment of mapad_amd.hip (device half; not a stand-alone header): the align_* kernels that build a batch's tracks from existing alignments
// (align_core.hpp).  Relies on what mapad_amd.hip defines in front of it: MAPAD_SLIM (beside the schedule kernels), BatchDev, and kScanTile of the collect
// section, whose compact_sums_kernel / compact_scan_tiles_kernel run between its two launches.  Launched from abi_align.hpp.

namespace {

// ---- tracks from alignments (align_core.hpp) -----------------------------------------------------------------------------------
// What a search, the collect above and records_kernel leave of a batch — hit_begin, one HitRec per read, the packed operations, one CoordRec per read — built from
// BAM fields instead: mapad_ctx_accumulate_alignments.  Two launches with the collect's scan between them:
//   align_count_kernel  a thread per read: the CIGAR-only classes and the track's length, as a "pool" the scan kernels above read (one hit per read, n_ops);
//   compact_sums_kernel + compact_scan_tiles_kernel + align_begin_kernel: ops_begin = the exclusive prefix sum (the third is compact_move_kernel without the move);
//   align_build_kernel  one wavefront per read, below.
struct AlignDev {
    const AlignIn* alns; const uint32_t* cigar; const uint8_t* md; const uint64_t* offsets;
    uint64_t n_reads;
    const uint64_t* contig_start; const uint64_t* contig_end;
    uint32_t n_contigs, min_mapq, start_at_end;
    uint32_t* hit_count; uint32_t* hit_first;  // [n_reads]: 1, r
    uint64_t* hit_begin; uint64_t* ops_begin;  // [n_reads + 1]
    HitRec* hits;                              // [n_reads]
    uint32_t* ops;
    CoordRec* coords;
    uint8_t* cls;                              // [n_reads]
    unsigned long long* counters;              // [ALN_CLASSES]
};
constexpr uint32_t kAlignBlock = 256;
__global__ void __launch_bounds__(kAlignBlock) align_count_kernel(AlignDev Q) {
    for (uint64_t r = (uint64_t)blockIdx.x * kAlignBlock + threadIdx.x; r < Q.n_reads; r += (uint64_t)gridDim.x * kAlignBlock) {
        const AlignIn a = Q.alns[r];
        uint32_t n_ops;
        uint64_t ref_len;
        const uint32_t cls = align_count(a, Q.cigar + a.cigar_off, Q.offsets[r + 1] - Q.offsets[r], Q.n_contigs, Q.min_mapq, n_ops, ref_len);
        HitRec h{};
        h.n_ops = n_ops;
        Q.hits[r] = h; Q.hit_count[r] = 1u; Q.hit_first[r] = (uint32_t)r; Q.cls[r] = (uint8_t)cls;
    }
}
__global__ void MAPAD_SLIM align_begin_kernel(AlignDev Q, const unsigned long long* __restrict__ tile_ops) {  // (tile-local exclusive scan: lane t owns reads 4t .. 4t+3 of the tile)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r0 = (uint64_t)blockIdx.x * kScanTile + 4 * lane;
    uint32_t o[4];
    unsigned long long to = 0, unused = 0;
    for (int q = 0; q < 4; ++q) { o[q] = r0 + q < Q.n_reads ? Q.hits[r0 + q].n_ops : 0; to += o[q]; }
    unsigned long long so = to;
    wave_scan2(so, unused, lane);
    unsigned long long ob = tile_ops[blockIdx.x] + so - to;
    for (int q = 0; q < 4; ++q) {
        const uint64_t r = r0 + q;
        if (r >= Q.n_reads) break;
        Q.hit_begin[r] = r; Q.ops_begin[r] = ob;
        ob += o[q];
    }
    if (blockIdx.x == 0 && lane == 0) Q.hit_begin[Q.n_reads] = Q.n_reads;
}

// One wavefront per read, four reads per block, a window of kAlignWindow reference positions per wavefront in LDS: "MD's byte at this offset of the alignment, 0 = a
// match" (align_core.hpp: the letter, kAlignDeleted on a deleted base) — where the two scans meet.  Longer alignments are walked window by window; the LDS per
// block does not depend on the read length.
//   * MD: 64 bytes per trip, a byte per lane.  align_md_advance says what the lane's byte adds to the reference offset (a number where its last digit stands, a
//     letter 1); a wave-wide scan gives every letter its offset; whether a letter is deleted is read off two ballots (is the nearest byte in front of it that is
//     no letter a ^?), with one carry bit between trips.  A trip that reaches beyond the window is taken again for the next window.
//   * CIGAR: 64 words per trip, a word per lane; a wave-wide scan gives every operation its first column, reference offset and SEQ index.
//   * Columns: 64 per trip, a column per lane, in reference order: the lane finds its operation (a loop over the trip's operations, one broadcast each: reads
//     have one to three), reads its reference byte out of the window and writes the operation word — slot k of a forward track, n - 1 - k of a reverse one, so
//     a trip writes 256 consecutive bytes.
// The read is walked twice: first without a write, to finish the classification (md_mismatch, off_contig) — nothing is written for a read that fails —, then to
// write.  Every lane of a wavefront takes the same branches (what they test is uniform), so the shuffles and ballots are always full.
constexpr uint32_t kAlignWindow = 256;
struct AlignWave {
    const uint8_t* md; uint32_t md_len;
    uint8_t* win;                    // the wavefront's window
    uint32_t lane;
    uint32_t md_t, md_off, md_del;   // the MD trip in turn: its first byte, the reference offset in front of it, whether a letter at its start would be deleted
    uint32_t w0, w1;                 // the window holds offsets [w0, w1)
    bool bad;
};
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v, uint32_t lane) {  // inclusive
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(v, d); if (lane >= (uint32_t)d) v += u; }
    return v;
}
// MD trips from the one in turn on, until MD ends or — RETIRE — a trip reaches beyond `upto` (it stays in turn) or — !RETIRE — a trip starts at or beyond `upto`;
// !RETIRE stores the letters that fall into the window.  A window is filled on a copy of the state: a trip stays in turn until a window starts at or behind its
// end, because the next window may begin in front of this one's end (it begins at a column trip's first offset).
template <bool RETIRE>
__device__ __forceinline__ void align_md_trips(AlignWave& W, uint32_t upto) {
    while (W.md_t < W.md_len) {
        if (!RETIRE && W.md_off >= upto) return;
        const uint32_t i = W.md_t + W.lane;
        const bool valid = i < W.md_len;
        bool bad = false;
        const uint8_t c = valid ? W.md[i] : (uint8_t)'0';
        const uint32_t cls = valid ? align_md_class(c) : (uint32_t)MD_OTHER;
        const uint32_t adv = valid ? align_md_advance(W.md, W.md_len, i, bad) : 0u;
        const uint32_t incl = wave_scan_u32(adv, W.lane);
        const uint32_t o = W.md_off + incl - adv;
        const unsigned long long carets = __ballot(valid && cls == MD_CARET), others = __ballot(valid && cls != MD_LETTER);
        if (__ballot(bad)) W.bad = true;
        const uint32_t end = W.md_off + (uint32_t)__shfl((int)incl, 63);
        if (!RETIRE && valid && cls == MD_LETTER && o >= W.w0 && o - W.w0 < kAlignWindow) {
            const unsigned long long in_front = others & ((1ull << W.lane) - 1ull);
            const uint32_t del = in_front ? (uint32_t)((carets >> (63 - __clzll((long long)in_front))) & 1ull) : W.md_del;
            W.win[o - W.w0] = (uint8_t)(damage_upper(c) | (del ? kAlignDeleted : 0u));
        }
        if (RETIRE && end > upto) return;
        if (others) W.md_del = (uint32_t)((carets >> (63 - __clzll((long long)others))) & 1ull);
        W.md_off = end; W.md_t += 64;
        if (end > 0x7FFFFFFFu) { W.bad = true; W.md_t = W.md_len; }  // (no alignment is that long: it cannot agree with the CIGAR)
    }
}
// the window moves to [from, from + kAlignWindow) and takes MD's letters there
__device__ __forceinline__ void align_window(AlignWave& W, uint32_t from) {
    reinterpret_cast<uint32_t*>(W.win)[W.lane] = 0u;  // 64 lanes x 4 bytes
    W.w0 = from; W.w1 = from + kAlignWindow;
    align_md_trips<true>(W, from);  // the trips that end at or in front of the window: none of their letters is needed again (offsets only grow)
    AlignWave T = W;
    align_md_trips<false>(T, W.w1);  // the trips that start inside it
    if (T.bad) W.bad = true;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the lanes read one another's bytes: LDS serves a wavefront's accesses in order, the compiler must keep them so
    __builtin_amdgcn_wave_barrier();
}
template <bool WRITE>
__device__ __forceinline__ bool align_wave_walk(const AlignIn& a, const uint32_t* __restrict__ cigar, const uint8_t* __restrict__ md, uint8_t* win, uint32_t lane, uint32_t L,
                                                uint32_t n_ops, uint32_t astart, uint32_t* __restrict__ out, uint32_t& ref_len) {
    AlignWave W{md, a.md_len, win, lane, 0, 0, 0, 0, 0, false};
    const bool backward = (a.flags & 0x10u) != 0;
    uint32_t c_carry = 0, r_carry = 0, s_carry = 0;
    bool disagree = false;
    for (uint32_t cb = 0; cb < a.n_cigar; cb += 64) {
        const uint32_t j = cb + lane, n_here = min(64u, a.n_cigar - cb);
        const uint32_t w = j < a.n_cigar ? cigar[j] : 0u, op = w & 15u, len = w >> 4;
        const uint32_t rl = op == CIG_I ? 0u : len, sl = op == CIG_D ? 0u : len;
        const uint32_t ci = wave_scan_u32(len, lane), ri = wave_scan_u32(rl, lane), si = wave_scan_u32(sl, lane);
        const uint32_t c0 = c_carry + ci - len, r0 = r_carry + ri - rl, s0 = s_carry + si - sl;
        const uint32_t c_end = c_carry + (uint32_t)__shfl((int)ci, 63);
        for (uint32_t k0 = c_carry; k0 < c_end; k0 += 64) {
            const uint32_t k = k0 + lane;
            const bool valid = k < c_end;
            uint32_t mine = 0;
            for (uint32_t jj = 1; jj < n_here; ++jj) if (k >= (uint32_t)__shfl((int)c0, (int)jj)) mine = jj;  // (first columns ascend: the last operation that starts at or before k)
            const uint32_t my_op = (uint32_t)__shfl((int)op, (int)mine), d = k - (uint32_t)__shfl((int)c0, (int)mine);
            const uint32_t o = (uint32_t)__shfl((int)r0, (int)mine) + (my_op == CIG_I ? 0u : d), s = (uint32_t)__shfl((int)s0, (int)mine) + (my_op == CIG_D ? 0u : d);
            const bool on_ref = valid && my_op != CIG_I;
            const unsigned long long need = __ballot(on_ref);
            if (need) {  // offsets ascend with the columns: the trip's lie in [first, last], fewer than 64 apart
                const uint32_t first = (uint32_t)__shfl((int)o, (int)(__ffsll((long long)need) - 1)), last = (uint32_t)__shfl((int)o, 63 - __clzll((long long)need));
                if (last >= W.w1 || first < W.w0) align_window(W, first);
            }
            const uint32_t ref = on_ref ? (uint32_t)win[(o - W.w0) & (kAlignWindow - 1)] : 0u;
            const uint32_t kind = my_op == CIG_I ? (uint32_t)OP_INS : align_column_kind(my_op, ref);
            if (__ballot(on_ref && kind == kAlignDisagree)) disagree = true;
            if (WRITE && valid) out[align_track_slot(n_ops, backward, k)] = align_op_word(kind, ref, s, L, backward, astart);
        }
        c_carry = c_end; r_carry += (uint32_t)__shfl((int)ri, 63); s_carry += (uint32_t)__shfl((int)si, 63);
    }
    ref_len = r_carry;
    if (WRITE) return true;
    align_md_trips<true>(W, 0xFFFFFFFFu);  // what is left of MD: every byte is looked at, and its reference length is known
    return !disagree && !W.bad && W.md_off == r_carry;
}
__global__ void __launch_bounds__(kAlignBlock) align_build_kernel(AlignDev Q) {
    __shared__ uint32_t windows[kAlignBlock / 64][kAlignWindow / 4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    constexpr uint32_t kWaves = kAlignBlock / 64;
    uint8_t* win = reinterpret_cast<uint8_t*>(windows[wave]);
    uint32_t n_cls[ALN_CLASSES] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // lane 0's count
    for (uint64_t r = (uint64_t)blockIdx.x * kWaves + wave; r < Q.n_reads; r += (uint64_t)gridDim.x * kWaves) {
        const AlignIn a = Q.alns[r];
        uint32_t cls = Q.cls[r];
        const uint32_t L = (uint32_t)(Q.offsets[r + 1] - Q.offsets[r]), n_ops = Q.hits[r].n_ops;
        const uint64_t ops_off = Q.ops_begin[r];
        if (cls == ALN_OK) {
            const uint32_t* cigar = Q.cigar + a.cigar_off;
            const uint8_t* md = Q.md + a.md_off;
            const uint32_t astart = align_start(L, Q.start_at_end != 0);
            uint32_t ref_len = 0;
            if (!align_wave_walk<false>(a, cigar, md, win, lane, L, n_ops, astart, nullptr, ref_len)) cls = ALN_MD_MISMATCH;
            else if (align_off_contig((uint64_t)a.pos0, ref_len, Q.contig_end[a.tid] - Q.contig_start[a.tid] + 1)) cls = ALN_OFF_CONTIG;
            else (void)align_wave_walk<true>(a, cigar, md, win, lane, L, n_ops, astart, Q.ops + ops_off, ref_len);
        }
        if (lane == 0) {
            HitRec h;
            CoordRec cr;
            align_records(cls, a, n_ops, (uint32_t)ops_off, cls == ALN_OK ? Q.contig_start[a.tid] : 0, h, cr);
            Q.hits[r] = h; Q.coords[r] = cr; Q.cls[r] = (uint8_t)cls;
#pragma unroll
            for (uint32_t k = 0; k < ALN_CLASSES; ++k) n_cls[k] += cls == k;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < ALN_CLASSES; ++k) if (n_cls[k]) atomicAdd(Q.counters + k, (unsigned long long)n_cls[k]);
    }
}

}  // namespace
