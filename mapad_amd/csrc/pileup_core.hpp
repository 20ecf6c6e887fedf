// pileup_core.hpp — the pileup: how often each of A, C, G, T is seen at every base of the reference in the alignments a run reports, and from that a consensus
// call per position and per-contig statistics.  What a user of an ancient-DNA mapper asks after damage and coverage (which base does the sample have here?),
// taken from what is on the device after a batch anyway — the records kernel's CoordRec, the reported alignment's edit track, the batch's bases and
// qualities — instead of from a coordinate sort and a CPU pileup over the BAM.  One source for pileup_kernel, pileup_call_kernel (mapad_amd.hip) and the
// host path (mapad_pileup_host_*): the tests compare the two, and both against a table built in numpy from POS, CIGAR, SEQ and QUAL.
//
// Definition.  S = n / 2 is the forward strand's text length (coverage_core.hpp); the accumulator is uint32 counts[S][4] over absolute forward-strand text
// positions (CoordOut::abs), bases in the order A, C, G, T, plus u64 scalars (below).  A cell wraps at 2^32; that is not checked.  The filters
// (PileupFilter: min_base_quality, mask5, mask3) are fixed while counts exist.  For one read of length L with the records kernel's `cr`:
//   * the read counts iff damage_read_counts(cr.mapped, cr.error, cr.x0, mode): mode 1 every mapped read, mode 2 only X0 == 1 (XT:U);
//   * only the reported alignment hits[cr.best] at cr.first counts, XA candidates do not;
//   * the operations are walked in reference order exactly as coverage_read walks them (coverage_ref_op); the offset o of an operation is the number of
//     non-insertion operations before it;
//   * a Match / Mismatch operation at offset o is one column at absolute position abs + o.  p = op & 0xFFFF is its 0-based position in the read as given
//     (5' -> 3', as in damage_column), q = upper(read[p]) its base, quals[p] its quality (raw Phred, as the API takes them).  The forward-strand base is q for
//     a forward record and q's complement for cr.first.backward.  The column goes to exactly one of, tested in this order:
//       (a) p >= L, or q not one of ACGT             -> columns_not_acgt
//       (b) p < mask5, or L - 1 - p < mask3          -> columns_masked       (so a read of L <= mask5 + mask3 bases is masked entirely; it still counts in reads)
//       (c) quals[p] < min_base_quality              -> columns_low_quality
//       (d) otherwise                                -> counts[abs + o][b] += 1, columns_counted += 1;
//   * a Deletion advances o and adds to deleted_columns only; an Insertion adds to insertions only.
// Every index is checked against S before it is written: an alignment that leaves [0, S] (never from record_coords) is reported, not written.
// Defined on the text as searched: positions the index replaced (OriginalSymbols) are ordinary, and the reference base is not consulted at all.
//
// Call rule, integer only, so that device and host cannot differ.  With d the sum of a position's four counts (u64) and best the largest: the call is that
// base iff d >= min_depth, best * 100 >= min_percent * d (in u64) and the maximum is unique; otherwise N.  min_depth >= 1, min_percent in 0..100.
// Per contig, for a given (min_depth, min_percent): sites_covered (d >= 1), sites_deep (d >= min_depth), sites_called, called[4] (calls by base),
// base_sum[4] (the sum of counts by base), max_depth (the largest d).
#pragma once
#include "coverage_core.hpp"

namespace mapad {

enum : uint32_t { PIL_READS = 0, PIL_READS_SEEN, PIL_COUNTED, PIL_NOT_ACGT, PIL_MASKED, PIL_LOW_QUAL, PIL_DELETED, PIL_INS, PIL_SCALARS };
// per-contig words of a summary
enum : uint32_t { PILC_COVERED = 0, PILC_DEEP, PILC_CALLED, PILC_CALLED_BASE, PILC_BASE_SUM = PILC_CALLED_BASE + 4, PILC_MAX_DEPTH = PILC_BASE_SUM + 4, PILC_WORDS };
constexpr uint32_t kPileupNoCall = 4;  // N

struct PileupFilter { uint32_t min_bq, mask5, mask3; };

// One Match / Mismatch operation: the scalar it adds to (PIL_COUNTED, PIL_NOT_ACGT, PIL_MASKED or PIL_LOW_QUAL); PIL_COUNTED: `b` is its forward-strand base 0..3.
MAPAD_HD uint32_t pileup_column(uint32_t op, const uint8_t* read, const uint8_t* quals, uint32_t L, bool backward, const PileupFilter& F, uint32_t& b) {
    const uint32_t p = op & 0xFFFFu;
    b = 0;
    if (p >= L) return PIL_NOT_ACGT;  // (never from the search; a caller-made result must not read beyond the read)
    const int qi = base_index((uint8_t)damage_upper(read[p]));
    if (qi > 3) return PIL_NOT_ACGT;
    if (p < F.mask5 || L - 1 - p < F.mask3) return PIL_MASKED;
    if ((uint32_t)quals[p] < F.min_bq) return PIL_LOW_QUAL;
    b = backward ? 3u - (uint32_t)qi : (uint32_t)qi;  // A <-> T, C <-> G
    return PIL_COUNTED;
}

// the call of one position: 0..3 = A, C, G, T, kPileupNoCall = N; d: its depth
MAPAD_HD uint32_t pileup_call(uint32_t a, uint32_t c, uint32_t g, uint32_t t, uint32_t min_depth, uint32_t min_percent, uint64_t& d) {
    d = (uint64_t)a + c + g + t;
    uint32_t best = a, at = 0, ties = 0;
    if (c > best) { best = c; at = 1; }
    if (g > best) { best = g; at = 2; }
    if (t > best) { best = t; at = 3; }
    ties = (uint32_t)(a == best) + (uint32_t)(c == best) + (uint32_t)(g == best) + (uint32_t)(t == best);
    const bool ok = d >= (uint64_t)min_depth && (uint64_t)best * 100ull >= (uint64_t)min_percent * d && ties == 1;
    return ok ? at : kPileupNoCall;
}
MAPAD_HD uint8_t pileup_letter(uint32_t call) { return call == 0 ? 'A' : call == 1 ? 'C' : call == 2 ? 'G' : call == 3 ? 'T' : 'N'; }

// One position into the per-contig words w[PILC_WORDS] of a summary (the host path; the device keeps them in registers).
template <typename Word>
MAPAD_HD uint32_t pileup_site(const uint32_t* cell, uint32_t min_depth, uint32_t min_percent, Word* w) {
    uint64_t d;
    const uint32_t call = pileup_call(cell[0], cell[1], cell[2], cell[3], min_depth, min_percent, d);
    w[PILC_COVERED] += d >= 1; w[PILC_DEEP] += d >= (uint64_t)min_depth; w[PILC_CALLED] += call != kPileupNoCall;
    if (call != kPileupNoCall) w[PILC_CALLED_BASE + call] += 1;
    for (uint32_t b = 0; b < 4; ++b) w[PILC_BASE_SUM + b] += cell[b];
    if (d > (uint64_t)w[PILC_MAX_DEPTH]) w[PILC_MAX_DEPTH] = (Word)d;
    return call;
}

// One read on one thread (the host path).  false: the alignment leaves [0, S] (never from record_coords; nothing is written then).
template <typename Counter>
MAPAD_HD bool pileup_read(const CoordRec& cr, const HitRec* hits, const uint32_t* ops, const uint8_t* read, const uint8_t* quals, uint32_t L, int mode, const PileupFilter& F,
                          uint64_t S, uint32_t* counts, Counter* scalars, bool dup = false) {
    scalars[PIL_READS_SEEN] += 1;
    if (dup) return true;  // a marked duplicate that is left out (dedup_core.hpp, mode 2): seen, not counted
    if (!damage_read_counts(cr.mapped, cr.error, cr.x0, mode)) return true;
    const HitRec& h = hits[cr.best];
    const uint32_t* t = ops + h.ops_off;
    const uint64_t abs = cr.first.abs;
    const bool backward = cr.first.backward != 0;
    if (abs > S || effective_len_hd(t, h.n_ops) > S - abs) return false;
    scalars[PIL_READS] += 1;
    uint64_t o = 0;
    for (uint32_t i = 0; i < h.n_ops; ++i) {
        const uint32_t op = coverage_ref_op(t, h.n_ops, backward, i), kind = op >> 24;
        if (kind == OP_INS) { scalars[PIL_INS] += 1; continue; }
        if (kind == OP_DEL) scalars[PIL_DELETED] += 1;
        else {
            uint32_t b;
            const uint32_t what = pileup_column(op, read, quals, L, backward, F, b);
            scalars[what] += 1;
            if (what == PIL_COUNTED) counts[(abs + o) * 4 + b] += 1;
        }
        o += 1;
    }
    return true;
}

}  // namespace mapad
