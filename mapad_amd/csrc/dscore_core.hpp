// dscore_core.hpp — the damage score: per read, the log-likelihood ratio (in bits) of its reported alignment under the mapper's damage model (sdm_get,
// host_models.hpp: -f / -t / -d / -s) against the same model with the damage term removed (sdm_get_null).  The per-read question an ancient-DNA pipeline asks of a
// contaminated library — does THIS read look ancient? — answered from what is on the device after a batch anyway.  One source for dscore_kernel (mapad_amd.hip), the
// host path (mapad_damage_score_host) and a stand-alone self-test (tests/emu/dscore_selftest.cpp).
//
// Definition, for one read of length L with the records kernel's `cr`:
//   * the read is scored iff cr.mapped && !cr.error; every other read has score 0 and scored = 0;
//   * the columns are those of damage_core.hpp: a Match or Mismatch operation of hits[cr.best] with p = op & 0xFFFF < L, q = upper(read[p]), r = the reference base
//     in read orientation (the op's byte for a Mismatch, q for a Match).  A column is informative iff (r, q) is one of C->C, C->T, G->G, G->A — the only pairs the two
//     models score differently; every other column, insertions, deletions, N and p >= L add nothing and load nothing;
//   * an informative column adds delta[p][quals[p]][cell] (level 0 where the table has one quality level), an int16 in units of 1/256 bit that the HOST has rounded
//     from the two models' f32 values (host_models.hpp: dscore_quantize, dscore_table) — the device never evaluates a transcendental;
//   * score_q (int32) is the sum: integers, so neither the order of addition nor the side it is computed on can change it.  The score is score_q / 256 bits;
//   * below the threshold iff scored && score_q < thr_q, thr_q = (int32)ceilf(threshold * 256) (host_models.hpp: dscore_threshold_q);
//   * the histogram has 128 bins of half a bit: bin = (clamp(score_q, -8192, 8191) + 8192) >> 7; bin 64 starts at score 0.
#pragma once
#include "damage_core.hpp"

namespace mapad {

constexpr uint32_t kDscoreBins = 128;  // MAPAD_DAMAGE_SCORE_BINS
enum : uint32_t { DS_READS_SEEN = 0, DS_READS_SCORED, DS_READS_BELOW, DS_COLUMNS, DS_SCORE_SUM, DS_SCALARS };  // DS_SCORE_SUM: two's complement of a signed sum
constexpr uint32_t kDscoreWords = DS_SCALARS + kDscoreBins;  // u64 counters of one accumulator: the scalars, then the bins
enum : uint32_t { DS_CC = 0, DS_CT = 1, DS_GG = 2, DS_GA = 3, kDscoreNoCell = 4 };

struct alignas(8) DscoreRow { int16_t v[4]; };  // one (position, quality level): C->C, C->T, G->G, G->A

MAPAD_HD bool dscore_read_scored(uint32_t mapped, uint32_t error) { return mapped && !error; }
// (reference base, read base), both upper case -> the cell, or kDscoreNoCell
MAPAD_HD uint32_t dscore_cell(uint32_t r, uint32_t q) {
    if (r == 'C') return q == 'C' ? (uint32_t)DS_CC : q == 'T' ? (uint32_t)DS_CT : (uint32_t)kDscoreNoCell;
    if (r == 'G') return q == 'G' ? (uint32_t)DS_GG : q == 'A' ? (uint32_t)DS_GA : (uint32_t)kDscoreNoCell;
    return kDscoreNoCell;
}
// one operation of the reported alignment: its cell (kDscoreNoCell: not informative) and, for an informative one, its read position
MAPAD_HD uint32_t dscore_column(uint32_t op, const uint8_t* read, uint32_t L, uint32_t& p) {
    const uint32_t kind = op >> 24;
    p = op & 0xFFFFu;
    if (kind == OP_INS || kind == OP_DEL || p >= L) return kDscoreNoCell;
    const uint32_t q = damage_upper(read[p]);
    const uint32_t r = kind == OP_MATCH ? q : damage_upper((op >> 16) & 0xFFu);
    return dscore_cell(r, q);
}
// the table row of (p, quality byte) in one length's table [L][nq]: one 8-byte load
MAPAD_HD int32_t dscore_delta(const DscoreRow* table, uint32_t nq, uint32_t p, uint32_t qual, uint32_t cell) {
    const DscoreRow row = table[(size_t)p * nq + (nq == 1 ? 0u : qual)];
    int32_t d = row.v[3];
    d = cell == DS_GG ? (int32_t)row.v[2] : d; d = cell == DS_CT ? (int32_t)row.v[1] : d; d = cell == DS_CC ? (int32_t)row.v[0] : d;
    return d;
}
MAPAD_HD uint32_t dscore_bin(int32_t score_q) {
    const int32_t c = score_q < -8192 ? -8192 : score_q > 8191 ? 8191 : score_q;
    return (uint32_t)(c + 8192) >> 7;
}

// One read on one thread (the host path).  `table`: the read length's table (nullptr: no column is informative); nq < 256 levels are indexed by the quality byte
// only where nq == 256 (quality_levels).  Returns score_q; `columns` gets the informative columns.
MAPAD_HD int32_t dscore_read(const HitRec& h, const uint32_t* ops, const uint8_t* read, const uint8_t* quals, uint32_t L, const DscoreRow* table, uint32_t nq, uint32_t& columns) {
    int32_t s = 0;
    columns = 0;
    if (!table) return 0;
    for (uint32_t i = 0; i < h.n_ops; ++i) {
        uint32_t p;
        const uint32_t cell = dscore_column(ops[h.ops_off + i], read, L, p);
        if (cell == kDscoreNoCell) continue;
        s += dscore_delta(table, nq, p, quals[p], cell);
        columns += 1;
    }
    return s;
}
// what one read adds to an accumulator acc[kDscoreWords] (the host path; the kernel keeps the same sums in registers and LDS)
template <typename Counter>
MAPAD_HD void dscore_account(bool scored, int32_t score_q, uint32_t columns, int32_t thr_q, Counter* acc) {
    acc[DS_READS_SEEN] += 1;
    if (!scored) return;
    acc[DS_READS_SCORED] += 1;
    acc[DS_READS_BELOW] += score_q < thr_q;
    acc[DS_COLUMNS] += columns;
    acc[DS_SCORE_SUM] += (Counter)(long long)score_q;
    acc[DS_SCALARS + dscore_bin(score_q)] += 1;
}

}  // namespace mapad
