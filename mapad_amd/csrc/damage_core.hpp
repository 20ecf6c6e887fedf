// damage_core.hpp — the damage profile: reference base -> read base counts by distance from the read's 5' and 3' end, over the alignments a run
// reports.  What a user of an ancient-DNA mapper looks at first (does the library show C->T / G->A excess at the ends?  were -f / -t / -d / -s the
// right ones?), taken from what is on the device after a batch anyway — the reported alignment's edit track, the reads, the records kernel's
// CoordRec — instead of from a second pass over the BAM.  One source for damage_kernel (mapad_amd.hip) and for the host path
// (mapad_damage_profile_host): the tests compare the two, and the host path against a table decoded from CIGAR / MD / SEQ.
//
// Definition, for one read of length L with the records kernel's `cr`:
//   * the read counts iff cr.mapped && !cr.error and, in mode 2 ("unique"), cr.x0 == 1 — the condition under which its record carries XT:U;
//   * of the reported hit hits[cr.best], every Match / Mismatch operation is one aligned column: p = op & 0xFFFF is the 0-based position in the read
//     as given (5' -> 3': the search's `j`, search_core.hpp), q = the read's base there.  A Mismatch carries the reference base in bits 16..23, in read
//     orientation (for a reverse-strand record to_bam_fields reverses the track and complements that base: record.rs:282-449, text_core.hpp:
//     bam_fields_hd), so no strand handling is needed here.  A Match carries NO base (record.rs:229 `Match(u16)`; its byte is 0): the reference base
//     is the read's own — a Match is only ever emitted for a read base that is one of ACGT (base_index, common.hpp);
//   * both bases are upper-cased; if both are one of ACGT the column adds 1 to counts[0][p][r][q] when p < P and 1 to counts[1][L - 1 - p][r][q] when
//     L - 1 - p < P (P = 32; a base of a short read may land in both tables) and 1 to aligned_bases whatever its position; otherwise (N in the read,
//     X in the text, a position outside the read) it adds 1 to skipped_bases;
//   * Insertion / Deletion operations add to insertions / deletions only.
// The profile is defined on the text as searched: ambiguity codes of the reference that the index replaced by a compatible base (OriginalSymbols,
// src/index/mod.rs), and that MD restores, are not consulted.
#pragma once
#include "postproc_core.hpp"

namespace mapad {

constexpr uint32_t kDamagePositions = 32;                          // MAPAD_DAMAGE_POSITIONS
constexpr uint32_t kDamageCells = 2 * kDamagePositions * 16;       // [end][distance][ref][read]
enum : uint32_t { DMG_READS = 0, DMG_READS_SEEN, DMG_ALIGNED, DMG_SKIPPED, DMG_INS, DMG_DEL, DMG_SCALARS };
constexpr uint32_t kDamageWords = kDamageCells + DMG_SCALARS;      // u64 counters of one accumulator: the cells, then the scalars
constexpr uint32_t kDamageNoCell = 0xFFFFFFFFu;

MAPAD_HD bool damage_read_counts(uint32_t mapped, uint32_t error, uint64_t x0, int mode) { return mapped && !error && (mode != 2 || x0 == 1); }
MAPAD_HD uint32_t damage_upper(uint32_t c) { return c >= 'a' && c <= 'z' ? c - 32u : c; }

// one operation of the reported alignment
struct DamageColumn {
    uint32_t what;          // DMG_ALIGNED, DMG_SKIPPED, DMG_INS or DMG_DEL: the scalar it adds to
    uint32_t cell5, cell3;  // DMG_ALIGNED: its cell in the 5' / 3' table, kDamageNoCell beyond the table
};
MAPAD_HD DamageColumn damage_column(uint32_t op, const uint8_t* read, uint32_t L) {
    DamageColumn c{DMG_SKIPPED, kDamageNoCell, kDamageNoCell};
    const uint32_t kind = op >> 24;
    if (kind == OP_INS) { c.what = DMG_INS; return c; }
    if (kind == OP_DEL) { c.what = DMG_DEL; return c; }
    const uint32_t p = op & 0xFFFFu;
    if (p >= L) return c;  // (never from the search; a caller-made result must not read beyond the read)
    const uint32_t q = damage_upper(read[p]);
    const uint32_t r = kind == OP_MATCH ? q : damage_upper((op >> 16) & 0xFFu);
    const int ri = base_index((uint8_t)r), qi = base_index((uint8_t)q);
    if (ri > 3 || qi > 3) return c;
    c.what = DMG_ALIGNED;
    const uint32_t rq = (uint32_t)(ri * 4 + qi), p3 = L - 1 - p;
    if (p < kDamagePositions) c.cell5 = p * 16 + rq;
    if (p3 < kDamagePositions) c.cell3 = (kDamagePositions + p3) * 16 + rq;
    return c;
}

// One read on one thread (the host path): adds into acc[kDamageWords].
template <typename Counter>
MAPAD_HD void damage_read(const CoordRec& cr, const HitRec* hits, const uint32_t* ops, const uint8_t* read, uint32_t L, int mode, Counter* acc, bool dup = false) {
    acc[kDamageCells + DMG_READS_SEEN] += 1;
    if (dup) return;  // a marked duplicate that is left out (dedup_core.hpp, mode 2): seen, not counted
    if (!damage_read_counts(cr.mapped, cr.error, cr.x0, mode)) return;
    acc[kDamageCells + DMG_READS] += 1;
    const HitRec& h = hits[cr.best];
    for (uint32_t i = 0; i < h.n_ops; ++i) {
        const DamageColumn c = damage_column(ops[h.ops_off + i], read, L);
        acc[kDamageCells + c.what] += 1;
        if (c.cell5 != kDamageNoCell) acc[c.cell5] += 1;
        if (c.cell3 != kDamageNoCell) acc[c.cell3] += 1;
    }
}

}  // namespace mapad
