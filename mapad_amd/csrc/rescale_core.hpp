// rescale_core.hpp — quality rescaling: the base qualities of a batch with the likely-damaged bases marked down, so that the next tool (a variant caller, a plain
// consensus) stops trusting a C->T two bases from a read's 5' end at Q37.  mapDamage's rescaling rule with this mapper's own damage model (sdm_prob,
// host_models.hpp: -f / -t / -d / -s) as the damage posterior.  One source for rescale_kernel (mapad_amd.hip), the host path (mapad_quality_rescale_host) and a
// stand-alone self-test (tests/emu/rescale_selftest.cpp).
//
// Definition, for one read of length L with the records kernel's `cr`:
//   * Which reads.  A read is rescaled iff dscore_read_scored(cr.mapped, cr.error).  Every other read keeps its qualities.
//   * Which columns.  The candidate columns are those of dscore_column: a Mismatch operation of hits[cr.best] with p = op & 0xFFFF < L, whose (reference base, read
//     base), upper-cased and in read orientation, is C->T (cell 0) or G->A (cell 1).  Matches, every other mismatch, insertions, deletions, N, and p >= L change
//     nothing and load nothing.
//   * What a column does.  A candidate column with quality byte q != 255 gets q' = table[p][q][cell], a uint8.  q == 255 (quality missing) stays 255.  Every read
//     position belongs to at most one Match/Mismatch operation.  The writes of a read therefore never meet.
//   * The table is built on the host only, in double, per prepared read length, as uint8 [L][256][2] (host_models.hpp: rescale_table).  The device does nothing
//     but a table load.  Let P_dam and P_null be the model's probability of that column with and without the damage term: linear probabilities, before the log
//     and before the epsilon clamp, evaluated in double from the f32 parameters (sdm_prob).  Then
//         pd = clamp((P_dam - P_null) / P_dam, 0, 1), the posterior that the mismatch is damage;
//         e  = 10^(-q/10), from the read's own q, also under ignore_base_quality;
//         e' = 1 - (1 - e)(1 - pd);
//         q' = min(q, floor(-10 log10(e') + 0.5)), and 0 where e' >= 1.
//     pd == 0 (no damage, or P_dam <= P_null) is e' = e: q' = q, taken without evaluating the logarithm.  So q' <= q always, the table is the identity without
//     damage, and on a single-stranded library G->A sees the -d rate at every position.
//   * The summary counts the reads seen and rescaled, the candidate columns by cell, the bases changed (q' != q), the sum of q - q', and the changed bases by
//     min(q', 63): integers, so neither the order of addition nor the side it is computed on can change it.
#pragma once
#include "dscore_core.hpp"

namespace mapad {

constexpr uint32_t kRescaleBins = 64;  // MAPAD_RESCALE_BINS
enum : uint32_t { RS_READS_SEEN = 0, RS_READS_RESCALED, RS_COLS_CT, RS_COLS_GA, RS_CHANGED, RS_DROP_SUM, RS_SCALARS };
constexpr uint32_t kRescaleWords = RS_SCALARS + kRescaleBins;  // u64 counters of one accumulator: the scalars, then the bins
enum : uint32_t { RS_CT = 0, RS_GA = 1, kRescaleNoCell = 2 };
constexpr uint32_t kRescaleRow = 256 * 2;  // bytes of one read position in a table: [quality byte][cell]

// one operation of the reported alignment: its cell (kRescaleNoCell: not a candidate) and, for a candidate, its read position — dscore_column's walk
MAPAD_HD uint32_t rescale_column(uint32_t op, const uint8_t* read, uint32_t L, uint32_t& p) {
    const uint32_t c = dscore_column(op, read, L, p);
    return c == DS_CT ? (uint32_t)RS_CT : c == DS_GA ? (uint32_t)RS_GA : (uint32_t)kRescaleNoCell;
}
// the new quality byte of a candidate column in one length's table [L][256][2]: one byte load, none for a missing quality
MAPAD_HD uint32_t rescale_lookup(const uint8_t* table, uint32_t p, uint32_t q, uint32_t cell) {
    return q == 255u ? 255u : (uint32_t)table[(size_t)p * kRescaleRow + q * 2u + cell];
}
MAPAD_HD uint32_t rescale_bin(uint32_t new_q) { return new_q < kRescaleBins - 1 ? new_q : kRescaleBins - 1; }

struct RescaleTally { uint32_t cols[2] = {0, 0}, changed = 0, drop = 0; };  // of one read (or, in the kernel, of one lane over its reads)

// One read on one thread (the host path).  `table`: the read length's table (nullptr: no column is a candidate).  `out` holds a copy of `quals` and gets the
// bytes that change; `bins` (kRescaleBins counters) the changed bases by their new quality.
template <typename Counter>
MAPAD_HD void rescale_read(const HitRec& h, const uint32_t* ops, const uint8_t* read, const uint8_t* quals, uint8_t* out, uint32_t L, const uint8_t* table, RescaleTally& t, Counter* bins) {
    if (!table) return;
    for (uint32_t i = 0; i < h.n_ops; ++i) {
        uint32_t p;
        const uint32_t cell = rescale_column(ops[h.ops_off + i], read, L, p);
        if (cell == kRescaleNoCell) continue;
        t.cols[cell] += 1;
        const uint32_t q = quals[p], nq = rescale_lookup(table, p, q, cell);
        if (nq == q) continue;
        out[p] = (uint8_t)nq;
        t.changed += 1; t.drop += q - nq;
        bins[rescale_bin(nq)] += 1;
    }
}
// what one read adds to the scalars of an accumulator acc[kRescaleWords] (the host path; the kernel keeps the same sums in registers and LDS)
template <typename Counter>
MAPAD_HD void rescale_account(bool rescaled, const RescaleTally& t, Counter* acc) {
    acc[RS_READS_SEEN] += 1;
    if (!rescaled) return;
    acc[RS_READS_RESCALED] += 1;
    acc[RS_COLS_CT] += t.cols[RS_CT]; acc[RS_COLS_GA] += t.cols[RS_GA];
    acc[RS_CHANGED] += t.changed; acc[RS_DROP_SUM] += t.drop;
}

}  // namespace mapad
