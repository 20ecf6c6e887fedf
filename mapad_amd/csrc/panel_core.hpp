// panel_core.hpp — pseudo-haploid genotypes at a fixed panel of biallelic SNPs: per panel site, how often each of A, C, G, T is seen on each strand in the
// alignments a run reports, and from that one call per panel row (one read drawn at random, or the majority), written as EIGENSTRAT by the CLI.  What
// population-genetic work on low-coverage ancient DNA uses instead of diploid calls; taken from what is on the device after a batch anyway instead of from a
// coordinate sort and a CPU pileup over the BAM.  One source for panel_kernel, panel_call_kernel (mapad_amd.hip), the host path (mapad_snp_panel_host_*) and
// tests/emu/panel_selftest.cpp: the tests compare device and host, and both against a table built in numpy from POS, CIGAR, SEQ, QUAL and the strand.
//
// Panel.  The caller gives n_rows rows (tid, pos0, ref, alt).  A row is placed iff 0 <= tid < n_contigs and pos0 < the contig's length; its absolute
// forward-strand position is x = contig_start + pos0 (the coordinate of CoordOut::abs).  The distinct x of the placed rows, ascending, are the slots;
// slot_of_row[n_rows] is kept on the host side of the accumulation (kPanelNoSlot for an unplaced row).  Two rows at one position share a slot and its counts
// and keep their own alleles.  The accumulation sees slots only.  A row has valid alleles iff upper(ref) and upper(alt) are both in ACGT and differ; it is a
// transition iff its alleles are {C, T} or {A, G}.
//
// Accumulator.  uint32 counts[n_slots][2][4]: strand s = cr.first.backward (0 forward, 1 reverse), forward-strand base A, C, G, T.  One cell is 32 bytes.
// A count wraps at 2^32; that is not checked.  u64 scalars (PAN_*).  For one read of length L with the records kernel's `cr`:
//   * reads_seen += 1; the read counts iff it is not left out (dedup_skip) and damage_read_counts(cr.mapped, cr.error, cr.x0, mode);
//   * only hits[cr.best] at cr.first counts; its reference span is effective_len_hd of its track; an alignment that leaves [0, S] is reported, not written;
//   * reads += 1; lo = the first slot with x >= abs (panel_lower_bound); slot_x[lo] >= abs + span: no slot under the read, done — the common case;
//   * reads_on_panel += 1; the operations are walked in reference order (coverage_ref_op), offset o = non-insertion operations before the column.  A Match /
//     Mismatch column at abs + o == some slot's x goes through pileup_column under this stage's own PileupFilter to exactly one of columns_counted (then
//     counts[slot][s][b] += 1), columns_not_acgt, columns_masked, columns_low_quality; a Deletion column on a slot adds to columns_deleted only.  Columns
//     that are on no slot, and insertions, add to nothing.
// A mapping-quality filter is not part of this: MAPQ is computed on the host from CoordRec::order after the stages have run; mode 2 (X0 == 1) is the filter
// the device has.
//
// Call rule (PanelRule: call 0 random draw / 1 majority, min_depth >= 1, transitions 0 keep / 1 missing / 2 single strand, seed), integer only, so that
// device and host cannot differ.  For row i (the caller's index — a call depends neither on the sort nor on batches, devices or the order of reads):
//   1. unplaced or invalid alleles -> missing;  2. a transition under transitions == 1 -> missing;
//   3. strands used: both; under transitions == 2 only s = 1 (reverse) for a {C, T} row and only s = 0 (forward) for an {A, G} row — the strand on which
//      deamination (C -> T as read, G -> A on the forward strand for a reverse read) cannot produce the other allele;
//   4. n_ref, n_alt: the cell's counts at the row's ref / alt base summed over the used strands, n = n_ref + n_alt (u64), other = the two remaining bases;
//   5. n < min_depth -> missing;
//   6. the draw: u = splitmix64 of seed + (i + 1) * 0x9E3779B97F4A7C15 (panel_mix), k = the high 64 bits of u * n; ref iff k < n_ref;
//   7. call == 0: the draw.  call == 1: ref if n_ref > n_alt, alt if n_ref < n_alt, the draw on a tie;
//   8. '2' for ref, '0' for alt, '9' for missing (EIGENSTRAT: copies of the first allele, pseudo-haploid).
// Summary words for one rule (PANS_*): rows; rows_unplaced; rows_bad_alleles (placed, invalid alleles); rows_transition (placed, valid, a transition).  Over
// the placed rows with valid alleles, strands as in 3 (a transition under transitions == 1 is observed on both strands and never called): rows_covered
// (n + other >= 1), obs_ref, obs_alt, obs_other (sums of n_ref, n_alt, other), max_depth (largest n + other); rows_called, called_ref, called_alt,
// transitions_called.
#pragma once
#include "pileup_core.hpp"

namespace mapad {

enum : uint32_t { PAN_READS_SEEN = 0, PAN_READS, PAN_ON_PANEL, PAN_COUNTED, PAN_NOT_ACGT, PAN_MASKED, PAN_LOW_QUAL, PAN_DELETED, PAN_SCALARS };
static_assert(PIL_NOT_ACGT == PIL_COUNTED + 1 && PIL_MASKED == PIL_COUNTED + 2 && PIL_LOW_QUAL == PIL_COUNTED + 3, "pileup_column's classes are consecutive");
// pileup_column's class -> this table's scalar
MAPAD_HD uint32_t panel_scalar_of(uint32_t what) { return PAN_COUNTED + (what - PIL_COUNTED); }
enum : uint32_t {
    PANS_ROWS = 0, PANS_UNPLACED, PANS_BAD_ALLELES, PANS_TRANSITION, PANS_COVERED, PANS_CALLED, PANS_CALLED_REF, PANS_CALLED_ALT, PANS_TRANSITIONS_CALLED,
    PANS_OBS_REF, PANS_OBS_ALT, PANS_OBS_OTHER, PANS_MAX_DEPTH, PANS_WORDS
};
constexpr uint32_t kPanelNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kPanelCell = 8;  // words of one slot: [2 strands][4 bases]
constexpr uint32_t kPanelLanes = 64;  // probes per round of the search = slots per window of the walk = operations per trip

struct PanelRule { uint32_t call, min_depth, transitions; uint64_t seed; };
MAPAD_HD bool panel_rule_ok(const PanelRule& R) { return R.call <= 1 && R.min_depth >= 1 && R.transitions <= 2; }

// ---- the search: the first slot with x >= target in ascending slot_x[n], 64 probes per round ---------------------------------------------------------
// The answer lies in [lo, hi] (every slot before lo is < target, every slot from hi on is >= target).  One round cuts [lo, hi) into at most 64 chunks of
// `step` slots; lane l probes the last slot of chunk l (panel_probe; false: the chunk is empty).  Ascending order makes "probe < target" true for the first c
// lanes and false after: the answer lies in chunk c, whose last slot need not be looked at again (panel_narrow).  The range shrinks to less than 1/64 per
// round: ceil(log64 n) rounds of one dependent load each, 4 for 1.2 M slots where a binary search takes 21.
MAPAD_HD uint64_t panel_step(uint64_t lo, uint64_t hi) { return (hi - lo + kPanelLanes - 1) / kPanelLanes; }
MAPAD_HD bool panel_probe(uint64_t lo, uint64_t hi, uint32_t lane, uint64_t& at) {
    const uint64_t step = panel_step(lo, hi), first = lo + (uint64_t)lane * step;
    at = first + step - 1 < hi ? first + step - 1 : hi - 1;
    return first < hi;
}
MAPAD_HD void panel_narrow(uint64_t& lo, uint64_t& hi, uint32_t c) {
    const uint64_t step = panel_step(lo, hi), a = lo + (uint64_t)c * step, b = lo + (uint64_t)(c + 1) * step - 1;
    lo = a < hi ? a : hi;
    hi = b < hi ? b : hi;
}
// the wavefront's search, lane by lane (the host path and the self-test; panel_kernel runs the same rounds with a ballot)
inline uint64_t panel_lower_bound(const uint64_t* slot_x, uint64_t n, uint64_t target, uint32_t* rounds = nullptr) {
    uint64_t lo = 0, hi = n;
    uint32_t k = 0;
    while (lo < hi) {
        uint32_t c = 0;
        for (uint32_t lane = 0; lane < kPanelLanes; ++lane) {
            uint64_t at;
            c += panel_probe(lo, hi, lane, at) && slot_x[at] < target;
        }
        panel_narrow(lo, hi, c);
        ++k;
    }
    if (rounds) *rounds = k;
    return lo;
}

// One read on one thread (the host path), arranged as the wavefront arranges it: trips of 64 operations, and per trip windows of 64 slots from lo on.
// false: the alignment leaves [0, S] (never from record_coords; nothing is written then).
template <typename Counter>
inline bool panel_read(const CoordRec& cr, const HitRec* hits, const uint32_t* ops, const uint8_t* read, const uint8_t* quals, uint32_t L, int mode, const PileupFilter& F,
                       uint64_t S, const uint64_t* slot_x, uint64_t n_slots, uint32_t* counts, Counter* scalars, bool dup = false) {
    scalars[PAN_READS_SEEN] += 1;
    if (dup) return true;  // left out (dedup_skip): seen, not counted
    if (!damage_read_counts(cr.mapped, cr.error, cr.x0, mode)) return true;
    const HitRec& h = hits[cr.best];
    const uint32_t* t = ops + h.ops_off;
    const uint64_t abs = cr.first.abs;
    const bool backward = cr.first.backward != 0;
    if (abs > S) return false;
    const uint64_t span = effective_len_hd(t, h.n_ops);
    if (span > S - abs) return false;
    scalars[PAN_READS] += 1;
    const uint64_t lo = panel_lower_bound(slot_x, n_slots, abs);
    if (lo >= n_slots || slot_x[lo] >= abs + span) return true;
    scalars[PAN_ON_PANEL] += 1;
    uint64_t carry = 0;  // non-insertion operations of the trips before this one
    for (uint32_t base = 0; base < h.n_ops; base += kPanelLanes) {
        uint32_t op_of[kPanelLanes];
        uint64_t o_of[kPanelLanes];
        bool column[kPanelLanes];
        uint64_t o = carry;
        for (uint32_t lane = 0; lane < kPanelLanes; ++lane) {
            const uint32_t i = base + lane;
            op_of[lane] = i < h.n_ops ? coverage_ref_op(t, h.n_ops, backward, i) : 0u;
            column[lane] = i < h.n_ops && (op_of[lane] >> 24) != OP_INS;
            o_of[lane] = o;
            o += column[lane];
        }
        const uint64_t x0 = abs + carry, x1 = abs + o;  // the trip's columns are [x0, x1)
        for (uint64_t w = lo; w < n_slots && slot_x[w] < x1; w += kPanelLanes)
            for (uint32_t j = 0; j < kPanelLanes && w + j < n_slots; ++j) {
                const uint64_t x = slot_x[w + j];
                if (x < x0 || x >= x1) continue;
                for (uint32_t lane = 0; lane < kPanelLanes; ++lane) {
                    if (!column[lane] || abs + o_of[lane] != x) continue;
                    if ((op_of[lane] >> 24) == OP_DEL) { scalars[PAN_DELETED] += 1; continue; }
                    uint32_t b;
                    const uint32_t what = pileup_column(op_of[lane], read, quals, L, backward, F, b);
                    scalars[panel_scalar_of(what)] += 1;
                    if (what == PIL_COUNTED) counts[((w + j) * 2 + (backward ? 1u : 0u)) * 4 + b] += 1;
                }
            }
        carry = o;
    }
    return true;
}

// ---- the call rule ----------------------------------------------------------------------------------------------------------------------------------
MAPAD_HD uint64_t panel_mix(uint64_t seed, uint64_t i) {
    uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
MAPAD_HD uint64_t panel_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}
// allele byte -> 0..3, 4 = not one of ACGT (either case)
MAPAD_HD uint32_t panel_allele(uint8_t c) { return (uint32_t)base_index((uint8_t)damage_upper(c)); }
MAPAD_HD bool panel_transition(uint32_t r, uint32_t a) { return (r ^ a) == 2u; }  // A(0) <-> G(2), C(1) <-> T(3)

// One row: its output byte; w[PANS_WORDS] (or nullptr) takes its part of the summary.  cell: the 8 words of the row's slot (not read for an unplaced row).
template <typename Word>
MAPAD_HD uint8_t panel_call_row(uint32_t slot, const uint32_t* cell, uint8_t ref, uint8_t alt, const PanelRule& R, uint64_t i, Word* w) {
    const uint32_t r = panel_allele(ref), a = panel_allele(alt);
    const bool placed = slot != kPanelNoSlot, valid = r < 4 && a < 4 && r != a;
    if (w) { w[PANS_ROWS] += 1; w[PANS_UNPLACED] += !placed; w[PANS_BAD_ALLELES] += placed && !valid; }
    if (!placed || !valid) return '9';
    const bool transition = panel_transition(r, a);
    const bool single = transition && R.transitions == 2;
    // {C, T}: the reverse strand only; {A, G}: the forward strand only
    const bool use_fwd = !single || (r & 1u) == 0, use_rev = !single || (r & 1u) == 1;
    uint64_t n_ref = 0, n_alt = 0, all = 0;
    if (use_fwd) { n_ref += cell[r]; n_alt += cell[a]; all += (uint64_t)cell[0] + cell[1] + cell[2] + cell[3]; }
    if (use_rev) { n_ref += cell[4 + r]; n_alt += cell[4 + a]; all += (uint64_t)cell[4] + cell[5] + cell[6] + cell[7]; }
    const uint64_t n = n_ref + n_alt, other = all - n;
    const bool open = !(transition && R.transitions == 1) && n >= (uint64_t)R.min_depth;
    bool is_ref = panel_mulhi(panel_mix(R.seed, i), n) < n_ref;  // the draw (n == 0: never open)
    if (R.call == 1 && n_ref != n_alt) is_ref = n_ref > n_alt;
    if (w) {
        w[PANS_TRANSITION] += transition; w[PANS_COVERED] += all >= 1;
        w[PANS_OBS_REF] += (Word)n_ref; w[PANS_OBS_ALT] += (Word)n_alt; w[PANS_OBS_OTHER] += (Word)other;
        if (all > (uint64_t)w[PANS_MAX_DEPTH]) w[PANS_MAX_DEPTH] = (Word)all;
        w[PANS_CALLED] += open; w[PANS_CALLED_REF] += open && is_ref; w[PANS_CALLED_ALT] += open && !is_ref; w[PANS_TRANSITIONS_CALLED] += open && transition;
    }
    return !open ? '9' : is_ref ? '2' : '0';
}

}  // namespace mapad
