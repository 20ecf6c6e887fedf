// mappability_core.hpp — how many places of the reference a k-mer can be put: the per-start rule of the mappability stage, shared by the kernels and the host path.
//
// For a start p of a contig the stage counts the loci of the k-mer K = seq[p, p + k): c(p) = sum of loci(N) over all N at Hamming distance <= e (e = 0 | 1)
// from K, where loci(N) = the FMD interval size of N — its occurrences in the index's text, forward strand, '$', reverse complement, '$' —, halved when N is
// its own reverse complement (such a string is found once per strand at the same place).  A start is valid when the whole k-mer lies inside the contig and the
// caller's sequence has only A, C, G, T (either case) there; an invalid start counts 0.  The byte stored is min(c, 255).
//
// One backward search per start: the chain steps from the k-mer's last base to its first with one rank-query pair per base (fmd_device.hpp: ext1_*).  With
// e = 1 the chain asks for all four extensions of a column at once (ext4_*): the three bases that are not the k-mer's own start a branch each, which then
// goes on exactly down to the first base and ends as soon as its interval is empty.  Only (lower, size) are kept: nothing here extends forward.
//
// The bases of a block of starts (kBlockStarts + k - 1 of them) are staged 2-bit-packed, 16 per word, with a validity bit each — in LDS by the kernel, in a
// small array by the host path —, so that both read a base the same way (Staged).
#pragma once
#include "fmd_device.hpp"

namespace mapad {
namespace mappability {

constexpr int kMaxK = 255;
constexpr int kBins = 9;                                  // histogram of c over the valid starts: 1, 2, 3-4, 5-8, 9-16, 17-32, 33-64, 65-128, >= 129
constexpr int kBlockStarts = 256;                         // starts of one block of the count kernel (64 quads x 4 starts) and of one unit of host work
constexpr int kStageBases = kBlockStarts + kMaxK - 1;     // the block's starts and the halo of the last of them
constexpr int kStageWords = (kStageBases + 15) / 16;
constexpr uint32_t kDefaultTile = 1u << 22;               // starts per tile of the device path (MAPAD_MAPPABILITY_TILE lowers it)
enum : int { SUM_VALID = 0, SUM_UNIQUE = 1, SUM_HIST = 2, SUM_MAJORITY = SUM_HIST + kBins, SUM_STRICT, SUM_WORDS };

// ASCII -> 0..3 for ACGT in either case, 4 otherwise
MAPAD_HD int base_code(uint8_t c) { return base_index((uint8_t)(c >= 'a' && c <= 'z' ? c - 'a' + 'A' : c)); }

// 16 bases at seq[0 .. 16) -> their packed word and validity bits; bases at or behind `avail` (the end of the contig) are invalid
MAPAD_HD void pack16(const uint8_t* seq, uint64_t avail, uint32_t& bases, uint32_t& valid) {
    uint32_t b = 0, v = 0;
    for (int i = 0; i < 16; ++i) {
        const int code = (uint64_t)i < avail ? base_code(seq[i]) : 4;
        if (code <= 3) { b |= (uint32_t)code << (2 * i); v |= 1u << i; }
    }
    bases = b; valid = v;
}

struct Staged {
    const uint32_t* base;   // 16 bases per word
    const uint16_t* valid;  // their validity bits
};
MAPAD_HD int staged_base(const Staged& s, int i) { return (int)((s.base[i >> 4] >> (2 * (i & 15))) & 3u); }
// every base of [i, i + k) is valid
MAPAD_HD bool staged_valid(const Staged& s, int i, int k) {
    const int end = i + k;
    while (i < end) {
        const int w = i >> 4, lo = i & 15, hi = end - 16 * w < 16 ? end - 16 * w : 16;
        const uint32_t mask = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
        if (((uint32_t)s.valid[w] & mask) != mask) return false;
        i = 16 * (w + 1);
    }
    return true;
}

// Which strings around K are their own reverse complement.  Only an even k has any.  With M = the pairs (i, k - 1 - i), i < k / 2, whose bases are NOT
// complementary: K itself is one iff M is empty; a neighbour with base b at column j is one iff M is the single pair that holds j and b complements the base
// of the pair's other column (every other pair has to be complementary already, and b differs from K[j], so j's pair is in M).
struct Palindromes {
    int pairs;  // -1 not looked at yet; else min(|M|, 2); odd k: 2
    int first;  // the smaller column of M's first pair
};
MAPAD_HD void palindromes_scan(const Staged& s, int p, int k, Palindromes& pal) {
    if (pal.pairs >= 0) return;
    pal.pairs = 2; pal.first = 0;
    if (k & 1) return;
    int n = 0;
    for (int i = 0; i < k / 2 && n < 2; ++i)
        if (staged_base(s, p + i) != 3 - staged_base(s, p + k - 1 - i)) { if (n == 0) pal.first = i; ++n; }
    pal.pairs = n;
}
MAPAD_HD bool palindrome_self(const Palindromes& pal) { return pal.pairs == 0; }
MAPAD_HD bool palindrome_neighbour(const Staged& s, int p, int k, const Palindromes& pal, int j, int b) {
    if (pal.pairs != 1) return false;
    const int other = k - 1 - pal.first;
    return (j == pal.first && b == 3 - staged_base(s, p + other)) || (j == other && b == 3 - staged_base(s, p + pal.first));
}

// four values, one per base, as scalars: picked with selects over values already read (a pick through a reference became a load at a run-time offset of a
// copy in scratch memory), so that nothing of a chain lives in an array with a run-time index
struct Four { uint64_t a, c, g, t; };
MAPAD_HD uint64_t pick4(uint64_t a, uint64_t c, uint64_t g, uint64_t t, int k) { uint64_t r = t; r = k == 2 ? g : r; r = k == 1 ? c : r; r = k == 0 ? a : r; return r; }
MAPAD_HD uint64_t pick4(Four v, int k) { return pick4(v.a, v.c, v.g, v.t, k); }

// The rank queries of the host path: one thread, the whole block per query.
struct ScalarQuery {
    MAPAD_HD void step1(const DevIndex& ix, uint64_t lower, uint64_t size, int b, uint64_t& new_lower, uint64_t& new_size) const {
        ext1_scalar(ix, lower, size, b, new_lower, new_size);
    }
    MAPAD_HD void step4(const DevIndex& ix, uint64_t lower, uint64_t size, Four& lo4, Four& sz4) const {
        Ext4 x;
        ext4_scalar(ix, lower, 0, size, x);
        lo4 = Four{x.lower[0], x.lower[1], x.lower[2], x.lower[3]};
        sz4 = Four{x.size[0], x.size[1], x.size[2], x.size[3]};
    }
};
#if defined(__HIPCC__)
// ... and of the kernel: the quad's four lanes serve one query (w = lane & 3); every input and output is quad-uniform.
struct QuadQuery {
    int w;
    __device__ __forceinline__ void step1(const DevIndex& ix, uint64_t lower, uint64_t size, int b, uint64_t& new_lower, uint64_t& new_size) const {
        ext1_quad(ix, lower, size, b, w, new_lower, new_size);
    }
    // ext4_quad_lane hands lane w the extension by base w: the three alternatives of a column come with the query the chain needs anyway
    __device__ __forceinline__ void step4(const DevIndex& ix, uint64_t lower, uint64_t size, Four& lo4, Four& sz4) const {
        ExtLane x;
        ext4_quad_lane(ix, lower, 0, size, w, x);
        lo4 = Four{quad_bcast64<0>(x.lower), quad_bcast64<1>(x.lower), quad_bcast64<2>(x.lower), quad_bcast64<3>(x.lower)};
        sz4 = Four{quad_bcast64<0>(x.size), quad_bcast64<1>(x.size), quad_bcast64<2>(x.size), quad_bcast64<3>(x.size)};
    }
};
#endif

// c(p) of the valid start p (an index into the staged bases), saturated at 255.  `steps` counts the extension steps taken (two rank queries each).
// e = 0 and not `full`: the chain stops as soon as its interval has size 1.  The caller's sequence is the index's reference, so the k-mer is known to occur:
// every longer suffix of it occurs too, the interval can only shrink to that one occurrence and never to none.  (A k-mer that is its own reverse complement
// is found on both strands, so none of its suffixes has size 1.)  `full` runs every chain to the k-mer's first base: then a valid start that counts 0 shows
// a sequence that is not the index's.
template <class Q>
MAPAD_HD uint32_t count_start(const DevIndex& ix, const Staged& s, int p, int k, int e, bool full, const Q& q, uint32_t& steps) {
    uint64_t lower = 0, size = ix.n, total = 0;
    Palindromes pal{-1, 0};
    for (int j = k - 1; j >= 0; --j) {
        const int t = staged_base(s, p + j);
        if (e) {
            Four lo4, sz4;
            q.step4(ix, lower, size, lo4, sz4);
            ++steps;
            for (int alt = 1; alt < 4; ++alt) {
                const int b = (t + alt) & 3;
                uint64_t bl = pick4(lo4, b), bs = pick4(sz4, b);  // K with base b at column j: exact from here on
                if (bs == 0) continue;
                for (int i = j - 1; i >= 0 && bs; --i) { q.step1(ix, bl, bs, staged_base(s, p + i), bl, bs); ++steps; }
                if (bs) {
                    palindromes_scan(s, p, k, pal);
                    total += palindrome_neighbour(s, p, k, pal, j, b) ? bs >> 1 : bs;
                }
            }
            lower = pick4(lo4, t); size = pick4(sz4, t);
        } else {
            q.step1(ix, lower, size, t, lower, size);
            ++steps;
        }
        if (size == 0) break;
        if (!e && !full && size == 1) break;
    }
    if (size > 1) { palindromes_scan(s, p, k, pal); total += palindrome_self(pal) ? size >> 1 : size; }
    else total += size;
    return total > 255 ? 255u : (uint32_t)total;
}

// ---- cover and masks ---------------------------------------------------------------------------------------------------------------------------------
// starts s in [max(0, x - k + 1), x] whose k-mer lies inside the contig of length len
MAPAD_HD uint32_t possible_starts(uint64_t x, uint32_t k, uint64_t len) {
    if (len < k) return 0;
    const uint64_t lo = x + 1 >= k ? x + 1 - k : 0, hi = x < len - k ? x : len - k;
    return hi >= lo ? (uint32_t)(hi - lo + 1) : 0u;
}
MAPAD_HD bool mask_majority(uint32_t cover, uint32_t possible) { return 2 * cover > possible; }
MAPAD_HD bool mask_strict(uint32_t cover, uint32_t possible) { return possible > 0 && cover == possible; }
MAPAD_HD int hist_bin(uint32_t c) {  // c >= 1
    int b = 0;
    for (uint32_t v = c - 1; v; v >>= 1) ++b;
    return b < kBins ? b : kBins - 1;
}
// set bits of positions [a, a + len) of a bit array
MAPAD_HD uint32_t bits_in_range(const uint64_t* words, int a, int len) {
    uint32_t n = 0;
    const int end = a + len;
    while (a < end) {
        const int w = a >> 6, lo = a & 63, hi = end - 64 * w < 64 ? end - 64 * w : 64;
        const uint64_t upto = hi == 64 ? ~0ull : (1ull << hi) - 1ull;
        n += (uint32_t)popc64(words[w] & upto & ~((1ull << lo) - 1ull));
        a = 64 * (w + 1);
    }
    return n;
}

}  // namespace mappability
}  // namespace mapad
