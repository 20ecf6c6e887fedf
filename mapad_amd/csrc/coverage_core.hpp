// coverage_core.hpp — depth of coverage: how often every base of the reference is covered by the alignments a run reports, and from that the per-contig
// breadth (bases covered at least once), mean and maximum depth and the depth histogram.  The other figure a user of an ancient-DNA mapper reads off a
// mapping first; taken from what is on the device after a batch anyway — the records kernel's CoordRec and the reported alignment's edit track — instead of
// from a sort and a second pass over the BAM.  One source for coverage_kernel and the finishing pass (mapad_amd.hip) and for the host path
// (mapad_coverage_host_*): the tests compare the two, and both against per-base depth built in numpy from CIGAR and POS.
//
// Definition.  S = n / 2 is the forward strand's text length; the accumulator is int32 diff[S + 1], a difference array over absolute forward-strand text
// positions (CoordOut::abs), plus u64 counters (the scalars below, then one reads counter per contig).  For one read with the records kernel's `cr`:
//   * the read counts iff damage_read_counts(cr.mapped, cr.error, cr.x0, mode): mode 1 every mapped read, mode 2 only X0 == 1 (XT:U);
//   * only the reported alignment hits[cr.best] at cr.first counts, XA candidates do not;
//   * reference order is track order for a forward record and reversed track order for cr.first.backward (bam_fields_hd: backward ? ops[n-1-i] : ops[i]);
//     the offset o of an operation is the number of non-insertion operations before it in reference order, eff their total (effective_len_hd);
//   * the read adds diff[abs] += 1 and diff[abs + eff] -= 1; every Deletion at offset o adds diff[abs + o] -= 1 and diff[abs + o + 1] += 1: match and
//     mismatch columns cover their reference base, deleted reference bases are not covered, insertions touch nothing (samtools depth without -J);
//   * contig_reads[cr.first.tid] += 1; covered_columns / deleted_columns / insertions count operations.
// depth[x] is the inclusive prefix sum of diff up to x.  contig_of_hd keeps an alignment inside its contig, so abs + eff <= S, the depth is never negative,
// it is 0 at every position outside the contigs (the sentinel behind the last one, diff[S]) and the whole array sums to 0.  The contigs tile the text without
// a gap, so the -1 of a read that ends on a contig's last base lands on the next contig's first position: the prefix sum needs no restart there and is NOT 0
// before a contig's first base when its neighbour's last base is covered.  Defined on the text as searched: positions the index replaced (OriginalSymbols)
// are ordinary.
#pragma once
#include "damage_core.hpp"

namespace mapad {

constexpr uint32_t kCoverageBins = 256;  // MAPAD_COVERAGE_BINS: depth histogram, the last bin is depth >= 255
enum : uint32_t { COV_READS = 0, COV_READS_SEEN, COV_COVERED, COV_DELETED, COV_INS, COV_SCALARS };  // counters[COV_SCALARS + tid] = contig_reads[tid]
constexpr uint32_t kCoverageNoContig = 0xFFFFFFFFu;

MAPAD_HD uint32_t coverage_bin(int64_t depth) { return depth >= (int64_t)(kCoverageBins - 1) ? kCoverageBins - 1 : (uint32_t)depth; }
// the i-th operation of a track of n in reference order
MAPAD_HD uint32_t coverage_ref_op(const uint32_t* ops, uint32_t n, bool backward, uint32_t i) { return backward ? ops[n - 1 - i] : ops[i]; }

// A stretch of at most `seg` text positions of one contig (tid), or of what lies between / behind the contigs (kCoverageNoContig: the sentinel and diff[S];
// summed like every other, counted nowhere).  The segments tile [0, S] in order: the finishing pass reduces each to one sum, scans the sums, and walks each
// again with its carry-in.
struct CoverageSeg { uint64_t start; uint32_t len, tid; };

// One read on one thread (the host path).  false: the alignment leaves [0, S] (never from record_coords; nothing is written then).
template <typename Counter>
MAPAD_HD bool coverage_read(const CoordRec& cr, const HitRec* hits, const uint32_t* ops, int mode, uint64_t S, int32_t* diff, Counter* counters, bool dup = false) {
    counters[COV_READS_SEEN] += 1;
    if (dup) return true;  // a marked duplicate that is left out (dedup_core.hpp, mode 2): seen, not counted
    if (!damage_read_counts(cr.mapped, cr.error, cr.x0, mode)) return true;
    const HitRec& h = hits[cr.best];
    const uint32_t* t = ops + h.ops_off;
    const uint64_t abs = cr.first.abs;
    if (abs > S || effective_len_hd(t, h.n_ops) > S - abs) return false;
    counters[COV_READS] += 1;
    counters[COV_SCALARS + (uint32_t)cr.first.tid] += 1;
    uint64_t o = 0;
    for (uint32_t i = 0; i < h.n_ops; ++i) {
        const uint32_t kind = coverage_ref_op(t, h.n_ops, cr.first.backward != 0, i) >> 24;
        if (kind == OP_INS) { counters[COV_INS] += 1; continue; }
        if (kind == OP_DEL) { counters[COV_DELETED] += 1; diff[abs + o] -= 1; diff[abs + o + 1] += 1; }
        else counters[COV_COVERED] += 1;
        o += 1;
    }
    diff[abs] += 1; diff[abs + o] -= 1;
    return true;
}

}  // namespace mapad
