// align_core.hpp — the alignment -> track rule: what a BAM record says of an alignment (contig, POS, strand, CIGAR, MD:Z, X0, AS) and the read as sequenced become
// the three things every accumulator stage reads of a batch — one HitRec, one CoordRec and the packed edit operations — as if a search had produced them.  It
// is the inverse of bam_fields_hd (text_core.hpp) and makes the nine stages usable on any BAM that carries MD.  One source for align_count_kernel and
// align_build_kernel (mapad_amd.hip: their lane-parallel walk is built from the primitives below), for the host path (mapad_alignment_tracks_host: align_read) and
// for tests/emu/align_selftest.cpp.
//
// The track a search leaves (search_core.hpp: extract_ops) is in READ order — ascending position in the read as sequenced —, which is reference order for a
// forward record and reversed reference order for a reverse one (coverage_ref_op).  An operation is kind << 24 | reference base << 16 | read position:
//   * Match / Mismatch / Insertion: the 0-based position of the base in the read as sequenced (for a 0x10 record L - 1 - its index in SEQ);
//   * Mismatch / Deletion: the reference base in READ orientation (for a 0x10 record the complement of MD's letter), upper case; Match and Insertion carry 0 (the
//     reference base of a Match column is the read's own);
//   * Deletion: the search writes the position it stood at.  With q read bases in front of the deletion in read order and the alignment started at position
//     `astart` (alignment_start_of: L for the models that start at the 3' end, L / 2 otherwise) that is q - 1 where q <= astart (found on the way down, behind the
//     base consumed last) and q behind it (found on the way up, in front of the base consumed next); kept inside 0 .. L - 1.  A deletion exactly at a middle start
//     can be either in a search's track; no stage reads this field.
// Rules: M, = and X columns are Match or Mismatch as MD says (= and X are not trusted over MD); I is an Insertion; D is a Deletion whose bases are MD's ^ run;
// MD letters are upper-cased; a zero-length number between tokens is legal, a number of more than kAlignMaxDigits digits or above 65535 is not (no read is that
// long); a letter directly behind a ^ run belongs to the run.  MD carries the ORIGINAL symbol of a reference position that held an ambiguity code, a search's
// track the base the index drew for it: this path takes what MD says, so such a Mismatch has the reference base N (or R, Y, ...), which every stage classes as
// it classes any non-ACGT reference base.
//
// A read gets exactly one class, the first of AlignClass that applies; any class but ALN_OK leaves the read seen, not counted (mapped = 0, n_ops = 0, nothing
// written to the ops array), exactly like an unmapped read of a search.
#pragma once
#include "coverage_core.hpp"
#include "text_core.hpp"

namespace mapad {

enum AlignClass : uint32_t {
    ALN_OK = 0,
    ALN_UNMAPPED,           // 0x4 set, tid < 0 or pos0 < 0
    ALN_BELOW_MIN_MAPQ,
    ALN_NO_MD,              // md_len == 0
    ALN_BAD_CONTIG,         // tid >= n_contigs
    ALN_UNSUPPORTED_CIGAR,  // any of S H N P (or an unknown operation), no CIGAR, or 2^31 columns and more
    ALN_LENGTH_MISMATCH,    // CIGAR query length != read length
    ALN_MD_MISMATCH,        // MD's reference length != CIGAR's, an MD mismatch or deletion token where the CIGAR has none or the other, or an unparsable MD
    ALN_OFF_CONTIG,         // pos0 + span beyond the contig's end
    ALN_CLASSES
};

// = mapad_alignment_t (include/mapad_amd.h)
struct AlignIn {
    int64_t pos0;
    uint64_t x0;            // 0: no X0 tag -> 1
    uint64_t cigar_off, md_off;
    int32_t tid;
    uint32_t n_cigar, md_len;
    float as_score;
    uint16_t flags;
    uint8_t mapq, pad0;
    uint32_t pad1;
};
static_assert(sizeof(AlignIn) == 56, "alignment record layout");

enum : uint32_t { CIG_M = 0, CIG_I = 1, CIG_D = 2, CIG_EQ = 7, CIG_X = 8 };
MAPAD_HD bool align_cigar_supported(uint32_t op) { return op == CIG_M || op == CIG_I || op == CIG_D || op == CIG_EQ || op == CIG_X; }
MAPAD_HD bool align_cigar_query(uint32_t op) { return op == CIG_M || op == CIG_I || op == CIG_EQ || op == CIG_X; }
MAPAD_HD bool align_cigar_ref(uint32_t op) { return op == CIG_M || op == CIG_D || op == CIG_EQ || op == CIG_X; }

// The CIGAR-only part of the classification (every class up to ALN_LENGTH_MISMATCH; ALN_OK: so far), the track's length and the alignment's span on the reference.
MAPAD_HD uint32_t align_count(const AlignIn& a, const uint32_t* cigar, uint64_t L, uint32_t n_contigs, uint32_t min_mapq, uint32_t& n_ops, uint64_t& ref_len) {
    n_ops = 0; ref_len = 0;
    if ((a.flags & 0x4u) || a.tid < 0 || a.pos0 < 0) return ALN_UNMAPPED;
    if ((uint32_t)a.mapq < min_mapq) return ALN_BELOW_MIN_MAPQ;
    if (a.md_len == 0) return ALN_NO_MD;
    if ((uint32_t)a.tid >= n_contigs) return ALN_BAD_CONTIG;
    if (a.n_cigar == 0) return ALN_UNSUPPORTED_CIGAR;
    uint64_t cols = 0, q = 0, r = 0;
    bool bad = false;
    for (uint32_t i = 0; i < a.n_cigar; ++i) {
        const uint32_t w = cigar[i], op = w & 15u;
        const uint64_t len = w >> 4;
        bad = bad || !align_cigar_supported(op);
        cols += len;
        if (align_cigar_query(op)) q += len;
        if (align_cigar_ref(op)) r += len;
    }
    if (bad || cols >= (1ull << 31)) return ALN_UNSUPPORTED_CIGAR;
    if (q != L) return ALN_LENGTH_MISMATCH;
    n_ops = (uint32_t)cols; ref_len = r;
    return ALN_OK;
}
MAPAD_HD bool align_off_contig(uint64_t pos0, uint64_t ref_len, uint64_t contig_len) { return pos0 >= contig_len || ref_len > contig_len - pos0; }

// ---- MD:Z ----
enum : uint32_t { MD_DIGIT = 0, MD_LETTER, MD_CARET, MD_OTHER };
constexpr uint32_t kAlignMaxDigits = 10;
constexpr uint32_t kAlignMaxNumber = 65535;
constexpr uint32_t kAlignDeleted = 0x80u;  // on a reference byte: the position is deleted from the read
MAPAD_HD uint32_t align_md_class(uint8_t c) {
    if (c >= '0' && c <= '9') return MD_DIGIT;
    if ((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z')) return MD_LETTER;
    return c == '^' ? MD_CARET : MD_OTHER;
}
// What byte i of md[0 .. n) adds to the reference offset: a letter 1, a number its value where its last digit stands, everything else 0.  `bad`: no MD holds
// this byte here (a foreign character, a ^ without a letter behind it, a number too long or too large).  Looks at most kAlignMaxDigits bytes back and one ahead,
// so that a lane can call it for its own byte.
MAPAD_HD uint32_t align_md_advance(const uint8_t* md, uint32_t n, uint32_t i, bool& bad) {
    const uint32_t c = align_md_class(md[i]);
    if (c == MD_OTHER) { bad = true; return 0; }
    if (c == MD_LETTER) return 1;
    if (c == MD_CARET) { if (i + 1 >= n || align_md_class(md[i + 1]) != MD_LETTER) bad = true; return 0; }
    if (i + 1 < n && align_md_class(md[i + 1]) == MD_DIGIT) return 0;
    uint64_t v = 0, mul = 1;
    uint32_t k = 0;
    for (uint32_t j = i;; --j) {
        if (align_md_class(md[j]) != MD_DIGIT) break;
        if (k == kAlignMaxDigits) { bad = true; return 0; }
        v += (uint64_t)(md[j] - '0') * mul; mul *= 10; k += 1;
        if (j == 0) break;
    }
    if (v > kAlignMaxNumber) { bad = true; return 0; }
    return (uint32_t)v;
}

// MD read one reference position at a time (the host path): 0 a match, the upper-cased letter a mismatch, kAlignDeleted | letter a deleted base
constexpr uint32_t kAlignMdEnd = 0xFFFFFFFFu;
struct AlignMd {
    const uint8_t* md;
    uint32_t n, i, run;
    bool in_del, bad;
};
MAPAD_HD AlignMd align_md_open(const uint8_t* md, uint32_t n) { return AlignMd{md, n, 0, 0, false, false}; }
MAPAD_HD uint32_t align_md_next(AlignMd& m) {
    for (;;) {
        if (m.bad) return kAlignMdEnd;
        if (m.run) { m.run -= 1; return 0; }
        if (m.i >= m.n) return kAlignMdEnd;
        const uint8_t c = m.md[m.i];
        const uint32_t cls = align_md_class(c);
        if (cls == MD_LETTER) { m.i += 1; return (m.in_del ? kAlignDeleted : 0u) | damage_upper(c); }
        if (cls == MD_DIGIT) {
            uint32_t j = m.i;
            while (j + 1 < m.n && align_md_class(m.md[j + 1]) == MD_DIGIT) ++j;
            m.run = align_md_advance(m.md, m.n, j, m.bad);
            m.i = j + 1; m.in_del = false;
            continue;
        }
        (void)align_md_advance(m.md, m.n, m.i, m.bad);  // a ^ (in front of a letter) or a foreign character
        m.in_del = true; m.i += 1;
    }
}

// ---- columns -> operations ----
MAPAD_HD uint32_t align_start(uint32_t L, bool start_at_end) { return start_at_end ? L : L / 2; }  // alignment_start_of (search_core.hpp)
// One column of the alignment, in reference order, as the operation a search's track would hold.  kind: OP_*; ref: MD's byte of the position (Mismatch and
// Deletion; kAlignDeleted is ignored); s: the column's index in SEQ — for a Deletion the number of SEQ bases in front of it.
MAPAD_HD uint32_t align_op_word(uint32_t kind, uint32_t ref, uint32_t s, uint32_t L, bool backward, uint32_t astart) {
    const uint32_t letter = ref & 0x7Fu;
    const uint32_t shown = backward ? (uint32_t)complement_hd((uint8_t)letter) : letter;
    if (kind == OP_DEL) {
        const uint32_t q = backward ? L - s : s;  // read bases in front of it in read order
        uint32_t p = q <= astart ? (q ? q - 1 : 0u) : q;
        if (L && p >= L) p = L - 1;
        return pack_op(OP_DEL, p, shown);
    }
    const uint32_t p = backward ? L - 1 - s : s;
    return pack_op(kind, p, kind == OP_MISMATCH ? shown : 0u);
}
// where the k-th operation in reference order stands in a track of n (the inverse of coverage_ref_op)
MAPAD_HD uint32_t align_track_slot(uint32_t n, bool backward, uint32_t k) { return backward ? n - 1 - k : k; }
// the kind of an M / = / X or D column whose reference byte (MD) is `ref`, or kAlignDisagree where MD has a deletion and the CIGAR none, or the other way round
constexpr uint32_t kAlignDisagree = 0xFFu;
MAPAD_HD uint32_t align_column_kind(uint32_t cigar_op, uint32_t ref) {
    if (cigar_op == CIG_D) return (ref & kAlignDeleted) ? (uint32_t)OP_DEL : kAlignDisagree;
    if (ref & kAlignDeleted) return kAlignDisagree;
    return ref ? (uint32_t)OP_MISMATCH : (uint32_t)OP_MATCH;
}

// The walk of one alignment on one thread (the host path): false = MD and CIGAR disagree or MD cannot be parsed.  WRITE: out[0 .. n_ops) gets the track.
template <bool WRITE>
MAPAD_HD bool align_walk(const AlignIn& a, const uint32_t* cigar, const uint8_t* md, uint32_t L, uint32_t n_ops, bool start_at_end, uint32_t* out) {
    const bool backward = (a.flags & 0x10u) != 0;
    const uint32_t astart = align_start(L, start_at_end);
    AlignMd m = align_md_open(md, a.md_len);
    uint32_t k = 0, s = 0;
    for (uint32_t i = 0; i < a.n_cigar; ++i) {
        const uint32_t op = cigar[i] & 15u, len = cigar[i] >> 4;
        for (uint32_t t = 0; t < len; ++t, ++k) {
            uint32_t word;
            if (op == CIG_I) { word = align_op_word(OP_INS, 0, s, L, backward, astart); s += 1; }
            else {
                const uint32_t ref = align_md_next(m);
                if (ref == kAlignMdEnd) return false;
                const uint32_t kind = align_column_kind(op, ref);
                if (kind == kAlignDisagree) return false;
                word = align_op_word(kind, ref, s, L, backward, astart);
                if (kind != OP_DEL) s += 1;
            }
            if (WRITE) out[align_track_slot(n_ops, backward, k)] = word;
        }
    }
    return align_md_next(m) == kAlignMdEnd && !m.bad;
}

// ---- the records ----
MAPAD_HD void align_records(uint32_t cls, const AlignIn& a, uint32_t n_ops, uint32_t ops_off, uint64_t contig_start, HitRec& h, CoordRec& cr) {
    const bool ok = cls == ALN_OK;
    const uint64_t x0 = a.x0 ? a.x0 : 1;
    h.lower = 0; h.lower_rev = 0; h.size = ok ? x0 : 0; h.score = ok ? a.as_score : 0.0f; h.n_ops = ok ? n_ops : 0; h.ops_off = ops_off; h.pad = 0;
    cr.mapped = ok ? 1u : 0u; cr.best = 0;
    cr.first = ok ? CoordOut{0, a.tid, (uint64_t)a.pos0, contig_start + (uint64_t)a.pos0, (a.flags & 0x10u) ? 1u : 0u, 0} : CoordOut{0, -1, 0, 0, 0, 0};
    cr.x0 = ok ? x0 : 0; cr.x1 = 0; cr.n_xa = 0; cr.n_order = 0;
    cr.xa[0] = CoordOut{0, -1, 0, 0, 0, 0}; cr.xa[1] = cr.xa[0];
    for (int k = 0; k < kMaxHits; ++k) cr.order[k] = 0;
    cr.error = 0;
}

// One read on one thread (the host path): the CIGAR-only classes, the walk without a write, the contig's end, the walk that writes ops[ops_off .. ops_off + n_ops),
// the records.  n_ops_reserved: what align_count said (the read's room in the ops array, kept also where a later class leaves it unwritten).  Returns the class.
MAPAD_HD uint32_t align_read(const AlignIn& a, const uint32_t* cigar_words, const uint8_t* md_bytes, uint32_t L, const uint64_t* contig_start, const uint64_t* contig_end,
                             uint32_t n_contigs, uint32_t min_mapq, bool start_at_end, uint32_t ops_off, uint32_t* ops, HitRec& h, CoordRec& cr) {
    uint32_t n_ops = 0;
    uint64_t ref_len = 0;
    const uint32_t* cigar = cigar_words + a.cigar_off;
    const uint8_t* md = md_bytes + a.md_off;
    uint32_t cls = align_count(a, cigar, L, n_contigs, min_mapq, n_ops, ref_len);
    if (cls == ALN_OK && !align_walk<false>(a, cigar, md, L, n_ops, start_at_end, nullptr)) cls = ALN_MD_MISMATCH;
    if (cls == ALN_OK && align_off_contig((uint64_t)a.pos0, ref_len, contig_end[a.tid] - contig_start[a.tid] + 1)) cls = ALN_OFF_CONTIG;
    if (cls == ALN_OK) (void)align_walk<true>(a, cigar, md, L, n_ops, start_at_end, ops + ops_off);
    align_records(cls, a, n_ops, ops_off, cls == ALN_OK ? contig_start[a.tid] : 0, h, cr);
    return cls;
}

}  // namespace mapad
