"""Worlds, reads and oracle wiring of the record-level parity tests (tests/test_gpu_records.py on the GPU: records_kernel + text_kernel; tests/test_records_host.py
through the host path): one table, two runners, like tests/sweep_util.py.

Every record the product builds from a hit list — flags, tid, POS, MAPQ, strand, AS / XS bits, NM, X0, X1, XT, CIGAR, MD, XA — is compared with the oracle's
intervals_to_record over the same hits (parity_util.oracle_records_from_product_hits, seed 0: the one seed the oracle's stand-in for rand::rng() matches).

World A: four contigs, about 54 kb, with what the post-search code treats specially: every ambiguity code (original symbols, on both strands and inside XA
         entries), an N run that stays 'X' and one that is replaced base by base, a contig shorter than the reads, repeats (hit intervals of many rows go
         through PrRange), a long contig name, and reads that are gapped, long (CIGAR / MD numbers of three digits) or straddle a contig end.
World B: hit lists built by the caller, up to kMaxHits = 20 hits per read with tied scores: the uploaded (non-resident) path, and enough record text and
         (score, size) pairs to outgrow the text kernel's initial pools."""
import ctypes as C
import os
import re

import numpy as np

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import synth
from oracle import binding as ob

from kat_util import resolve_params
from parity_util import DAMAGE, NO_DAMAGE, canonical_records, compare_records, oracle_records_from_product_hits
from sweep_util import pack

SEED = 0  # oracle/capi.cpp: seed_for == postproc_core.hpp: seed_for_hd(0, ...)
PRESETS = {"no_damage": NO_DAMAGE, "damage": DAMAGE}
CODES = "NRYKMSWBDHVU"


class RecordWorld:
    """One reference text: the product's index and the oracle's index over the same BWT, with the product's suffix-array samples under the oracle's own LF walk,
    the contig table, and the original symbol of every position of the upper-cased input that is not A, C, G or T."""

    def __init__(self, contigs):
        had = os.environ.pop("MAPAD_INDEX_FIXED_REPLACEMENT", None)  # the real StdRng draws take part
        try:
            pidx = mapad_amd.Index.build([(n, s.tobytes()) for n, s in contigs])
        finally:
            if had is not None:
                os.environ["MAPAD_INDEX_FIXED_REPLACEMENT"] = had
        self._wire(pidx, contigs, 32)

    @classmethod
    def from_index(cls, pidx, contigs, sa_rate):
        """The same wiring over a product index that exists already (one opened from disk); sa_rate: the sampling rate of that index's suffix array."""
        self = cls.__new__(cls)
        self._wire(pidx, contigs, sa_rate)
        return self

    def _wire(self, pidx, contigs, sa_rate):
        self.pidx = pidx
        self.contigs = contigs
        self.starts = np.concatenate([[0], np.cumsum([len(s) for _, s in contigs])]).astype(np.int64)
        self.written = np.concatenate([s for _, s in contigs])
        upper = np.frombuffer(self.written.tobytes().upper(), np.uint8)
        self.is_code = ~np.isin(upper, np.frombuffer(b"ACGT", np.uint8))
        self.oidx = ob.OracleIndex.from_bwt(self.pidx.bwt(), "$ACGTX", 128)
        sample, er, ev = self.pidx.sampled_sa()
        self.oidx.set_sampled_sa(sample, sa_rate, er, ev)
        for k, (name, s) in enumerate(contigs):
            self.oidx.add_contig(int(self.starts[k]), int(self.starts[k]) + len(s) - 1, name)
        for p in np.flatnonzero(self.is_code):
            self.oidx.set_original_symbol(int(p), chr(upper[p]))

    def oracle_canon(self, preset, res, batch):
        orecs, otext = oracle_records_from_product_hits(self.oidx, ob.make_params(resolve_params(PRESETS[preset])), res, *batch, n_threads=2)
        return canonical_records(orecs, otext, oracle_side=True)


def params(preset):
    return mapad_amd.make_params(resolve_params(PRESETS[preset]))


def differing(recs_text, ocanon, lo=0, hi=None):
    """product (records, text) of reads [lo, hi) of a batch against the oracle's canonical records of the whole batch -> compare_records' triple"""
    recs, text = recs_text[:2]
    hi = len(ocanon[0]) if hi is None else hi
    assert len(recs) == hi - lo
    of, ot = ocanon
    first = [np.concatenate([[0], np.cumsum(lens)]) for lens, _ in ot]
    sub = (of[lo:hi], [(lens[lo:hi], b[int(f[lo]):int(f[hi])]) for (lens, b), f in zip(ot, first)])
    return compare_records(canonical_records(recs, text, oracle_side=False), sub)


def report(first, per_field, what=""):
    """compare_records' findings as an assertion message (a string: pytest prints it whole)"""
    return (f"{what}: " if what != "" else "") + f"first differing reads {first}; reads that differ by field: { {k: v for k, v in per_field.items() if v} }"


def _cat(batches):
    seqs = np.concatenate([b[0] for b in batches])
    quals = np.concatenate([b[1] for b in batches])
    offs = [np.zeros(1, np.uint64)]
    for b in batches:
        offs.append(b[2][1:] + offs[-1][-1])
    return seqs, quals, np.concatenate(offs).astype(np.uint64)


# ---- world A ------------------------------------------------------------------------------------------------------------------------------------------------
A_IUPAC = (5_000, 9_000)    # c0: one code every 37 bases
A_X_RUN = (12_000, 12_025)  # c0: 25 N, stays 'X'
A_N_RUN = (15_000, 15_019)  # c0: 19 N, replaced base by base: 19 consecutive original symbols
A_LOWER = (20_000, 20_400)  # c0: lower case in the input
A_REP_NAME = "repeat_contig_with_a_name_of_about_48_characters"
A_C3_RC = (3_000, 4_200)    # c3: the reverse complement of the clean c0[5000:6200]
A_C3_FWD = (10_000, 10_400)  # c3: a forward copy of the clean c0[7000:7400]
A_C3_TANDEM = (14_000, 18_000)  # c3: (ACGTTGCA) x 500 — its own reverse complement up to a rotation: about a thousand rows per exact hit


def world_a():
    """-> (RecordWorld, clean): `clean` is the concatenated text before the codes were written into it; every read is cut from it"""
    c0 = synth.genome(30_000, seed=101)
    unit = synth.genome(600, seed=102)
    rep = np.concatenate([np.tile(unit, 5), synth.genome(300, seed=103), synth.revcomp(unit), unit[:300]])
    tiny = synth.genome(60, seed=104)
    c3 = synth.genome(20_000, seed=105)
    c3[A_C3_RC[0]:A_C3_RC[1]] = synth.revcomp(c0[5_000:6_200])
    c3[A_C3_FWD[0]:A_C3_FWD[1]] = c0[7_000:7_400]
    c3[A_C3_TANDEM[0]:A_C3_TANDEM[1]] = np.tile(np.frombuffer(b"ACGTTGCA", np.uint8), 500)
    clean = np.concatenate([c0, rep, tiny, c3])
    w0 = c0.copy()
    for k, p in enumerate(range(A_IUPAC[0], A_IUPAC[1], 37)):
        w0[p] = ord(CODES[k % len(CODES)])
    w0[A_X_RUN[0]:A_X_RUN[1]] = ord("N")
    w0[A_N_RUN[0]:A_N_RUN[1]] = ord("N")
    w0[A_LOWER[0]:A_LOWER[1]] = np.frombuffer(w0[A_LOWER[0]:A_LOWER[1]].tobytes().lower(), np.uint8)
    assert len(A_REP_NAME) == 48
    return RecordWorld([("c0", w0), (A_REP_NAME, rep), ("tiny", tiny), ("c3", c3)]), clean


def _windows(clean, lo, hi, rng):
    """50-base windows in steps of 3 from the one that ends on base `lo` to the one that starts on base `hi - 1`, on both strands -> (reads, quals, sources)"""
    reads, src = [], []
    for s in range(max(lo - 49, 0), min(hi, len(clean) - 50), 3):
        w = clean[s:s + 50]
        reads += [w.copy(), synth.revcomp(w)]
        src += [(s, 0), (s, 1)]
    return reads, [rng.integers(20, 41, 50).astype(np.uint8) for _ in reads], src


def reads_a(world, clean):
    """-> (batch, straddlers): the natural reads, then the hand-laid 50-base windows across every contig junction and both N runs; straddlers = (read indices,
    the windows' start on the concatenated text, their strand)"""
    s = world.starts
    rep0, c3 = int(s[1]), int(s[3])
    parts = [
        synth.reads(clean, 900, 50, seed=201, qual_range=(20, 40)),                                                              # from everywhere
        synth.reads(clean[A_IUPAC[0] - 100:A_IUPAC[1] + 100], 500, 50, seed=202, qual_range=(20, 40), exo_frac=0.0, len_range=(30, 90), indel_frac=0.5),
        synth.reads(clean[rep0:int(s[2])], 300, 50, seed=203, qual_range=(20, 40), exo_frac=0.0, len_range=(30, 70)),            # the repeat
        synth.reads(clean[c3 + A_C3_RC[0]:c3 + A_C3_RC[1]], 200, 50, seed=204, qual_range=(20, 40), exo_frac=0.0, len_range=(40, 80), indel_frac=0.5),
        synth.reads(clean[c3 + A_C3_FWD[0]:c3 + A_C3_FWD[1]], 60, 50, seed=205, qual_range=(20, 40), exo_frac=0.0, len_range=(40, 80), indel_frac=0.5),
        synth.reads(clean[c3 + A_C3_TANDEM[0] - 60:c3 + A_C3_TANDEM[1] + 60], 40, 50, seed=206, qual_range=(20, 40), exo_frac=0.0, len_range=(30, 70)),
        synth.reads(clean, 30, 50, seed=207, qual_range=(20, 40), exo_frac=0.0, len_range=(120, 400)),                             # CIGAR / MD numbers of three digits
        synth.reads(clean[int(s[2]):c3], 12, 40, seed=209, qual_range=(20, 40), exo_frac=0.0, len_range=(30, 45)),                 # inside the 60-base contig
    ]
    natural = _cat(parts)
    rng = np.random.default_rng(208)
    reads, quals, src = [], [], []
    for lo, hi in [(int(j), int(j)) for j in s[1:-1]] + [A_X_RUN, A_N_RUN]:
        r, q, at = _windows(clean, lo, hi, rng)
        reads += r; quals += q; src += at
    batch = _cat([natural, pack(reads, quals)])
    n0 = len(natural[2]) - 1
    return batch, (np.arange(n0, n0 + len(src)), np.array([a for a, _ in src], np.int64), np.array([b for _, b in src], np.uint8))


def _strings(recs, text):
    t = np.asarray(text, np.uint8).tobytes()
    cut = lambda off, ln: [t[int(o):int(o) + int(k)].decode() for o, k in zip(off, ln)]  # noqa: E731
    return cut(recs["cigar_off"], recs["cigar_len"]), cut(recs["md_off"], recs["md_len"]), cut(recs["xa_off"], recs["xa_len"])


def edge_counts_a(world, recs, text, straddlers, hit_begin):
    """How often the product's records (arrays of hits_to_records(..., as_arrays=True)) of world A's batch meet what the world was built for; hit_begin: of the
    result they were made from."""
    m = recs["mapped"] != 0
    cigar, md, xa = _strings(recs, text)
    idx = np.flatnonzero(m)
    at, start, strand = straddlers
    absolute = world.starts[np.where(m, recs["tid"], 0)] + recs["pos"]
    moved = ~m[at] | (absolute[at] != start) | (recs["reverse"][at] != strand)
    has_hits = np.diff(hit_begin.astype(np.int64)) > 0
    return dict(reads=len(recs), mapped=int(m.sum()),
                md_code=sum(bool(re.search(r"[^0-9ACGT^]", md[i])) for i in idx),
                md_code_reverse=sum(bool(re.search(r"[^0-9ACGTN^]", md[i])) and bool(recs["reverse"][i]) for i in idx),
                xa_code=sum(any(re.search(r"[^0-9ACGT^]", e.split(",")[3]) for e in xa[i].split(";") if e) for i in idx),  # a code in the MD of an XA entry
                cigar_3_digits=sum(bool(re.search(r"\d{3}", cigar[i])) for i in idx),
                md_3_digits=sum(bool(re.search(r"\d{3}", md[i])) for i in idx),
                gapped=sum(bool(re.search(r"[ID]", cigar[i])) for i in idx),
                tids=sorted(set(recs["tid"][m].tolist())),
                with_xa=int((recs["xa_len"][m] > 0).sum()),
                xa_long_name=sum(A_REP_NAME in xa[i] for i in idx),
                x0_ge_3=int((recs["x0"][m] >= 3).sum()),
                x0_ge_300=int((recs["x0"][m] >= 300).sum()),
                reverse_share=float((recs["reverse"][m] != 0).mean()),
                straddlers=len(at), straddlers_moved=int(moved.sum()), straddlers_unmapped=int((~m[at]).sum()),
                # a straddler that has hits and no record: every hit was popped and none has a coordinate inside one contig (record_coords: `if (n_bc == 0) continue`)
                straddlers_hits_without_coordinate=int((has_hits[at] & ~m[at]).sum()), straddlers_mapped_elsewhere=int((m[at] & moved).sum()))


def check_reach_a(c):
    """Conditions, not measurements: each at roughly half of what the host path yields for this world (the yield beside it; tests/test_records_host.py prints them)."""
    assert c["md_code"] >= A_REACH["md_code"] and c["md_code_reverse"] >= A_REACH["md_code_reverse"] and c["xa_code"] >= A_REACH["xa_code"], c
    assert c["cigar_3_digits"] >= A_REACH["cigar_3_digits"] and c["md_3_digits"] >= A_REACH["md_3_digits"] and c["gapped"] >= A_REACH["gapped"], c
    assert c["tids"] == [0, 1, 2, 3], c
    assert c["with_xa"] >= A_REACH["with_xa"] and c["xa_long_name"] >= A_REACH["xa_long_name"] and c["x0_ge_3"] >= A_REACH["x0_ge_3"] and c["x0_ge_300"] >= A_REACH["x0_ge_300"], c
    assert c["reverse_share"] > 0.3 and c["straddlers_moved"] >= 1, c
    assert c["straddlers_hits_without_coordinate"] >= A_REACH["straddlers_hits_without_coordinate"] and c["straddlers_mapped_elsewhere"] >= A_REACH["straddlers_mapped_elsewhere"], c


# the host path yields, under no_damage / damage: md_code 191 / 190, md_code_reverse 87 / 86, xa_code 106 / 94, cigar_3_digits 26 / 26, md_3_digits 17 / 17, gapped 71 / 74,
# with_xa 566 / 552, xa_long_name 347 / 347, x0_ge_3 440 / 440, x0_ge_300 97 / 97 (the tandem repeat), reverse_share 0.47, 190 of 198 straddlers not at their source:
# 186 unmapped — 98 of them with hits of which none has a coordinate inside one contig (the windows across the contig joins), 88 without a hit (the windows over the N runs,
# cut from the clean text) — and 4 mapped elsewhere
A_REACH = dict(straddlers_hits_without_coordinate=49, straddlers_mapped_elsewhere=2, md_code=95, md_code_reverse=40, xa_code=47, cigar_3_digits=13, md_3_digits=8, gapped=35, with_xa=270, xa_long_name=170, x0_ge_3=220, x0_ge_300=45)


def ungapped_text_check_input(world, recs, offsets):
    """The records with every read unmapped whose alignment, taken as ungapped, touches a position that held an ambiguity code: what is left lies on stretches where
    the indexed text is the clean text, and parity_util.check_ungapped_records_against_the_text applies."""
    m = recs["mapped"] != 0
    lens = np.diff(offsets.astype(np.int64))
    cum = np.concatenate([[0], np.cumsum(world.is_code)])
    a = np.where(m, world.starts[np.where(m, recs["tid"], 0)] + recs["pos"], 0)
    touched = cum[np.minimum(a + lens, len(world.is_code))] - cum[a] > 0
    out = recs.copy()
    out["mapped"] = m & ~touched
    return out


# ---- world B ------------------------------------------------------------------------------------------------------------------------------------------------
B_NAME = "b_" + "a_contig_name_that_is_long_enough_to_make_XA_entries_outgrow_the_initial_text_pool_" * 2  # every XA entry carries it
B_READS = 1000
B_PRESET = "damage"


def world_b():
    """a 300 bp unit in 12 copies, each with about 3 % substitutions of its own, 200 random bases between them -> (RecordWorld, text, the copies' starts)"""
    rng = np.random.default_rng(301)
    unit = synth.genome(300, seed=302)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    parts, at, starts = [synth.genome(200, seed=303)], 200, []
    for k in range(12):
        c = unit.copy()
        sub = rng.random(300) < 0.03
        c[sub] = acgt[(np.searchsorted(acgt, c[sub]) + rng.integers(1, 4, int(sub.sum()))) & 3]
        starts.append(at)
        parts += [c, synth.genome(200, seed=304 + k)]
        at += 500
    text = np.concatenate(parts)
    return RecordWorld([(B_NAME, text)]), text, starts


def reads_b(text, starts):
    parts = [synth.reads(text[s:s + 300], (B_READS + 11) // 12, 50, seed=320 + k, qual_range=(20, 40), exo_frac=0.0) for k, s in enumerate(starts)]
    seqs, quals, offsets = _cat(parts)
    n = B_READS
    return seqs[:int(offsets[n])], quals[:int(offsets[n])], offsets[:n + 1]


def list_lengths_b(n):
    """every second read asks for the full 20 hits, the others cycle over 1 ... 20"""
    i = np.arange(n)
    return np.where(i % 2 == 1, 20, (i // 2) % 20 + 1)


class CallerResult:
    """A mapad_batch_result_t laid out by the caller (no private half: the library uploads its hits), with the numpy arrays it points into.  Has what both the
    product's converters (`_cptr`) and parity_util.oracle_records_from_product_hits (hit_begin, hits_arr, ops) read."""

    def __init__(self, hit_begin, hits_arr, ops):
        self.hit_begin = np.ascontiguousarray(hit_begin, np.uint64)
        self.hits_arr = np.ascontiguousarray(hits_arr, mb.HIT_DTYPE)
        self.ops = np.ascontiguousarray(ops, np.uint32)
        self.n_reads, self.n_hits, self.n_ops = len(self.hit_begin) - 1, len(self.hits_arr), len(self.ops)
        # what the kernels rely on without a check of their own
        hb = self.hit_begin.astype(np.int64)
        assert hb[0] == 0 and hb[-1] == self.n_hits and (np.diff(hb) >= 0).all() and (np.diff(hb) <= 20).all()
        n_ops = self.hits_arr["n_ops"].astype(np.int64)
        assert (self.hits_arr["ops_offset"].astype(np.int64) + n_ops <= self.n_ops).all()
        assert (self.hits_arr["size"] >= 1).all()
        self.status = np.zeros(max(self.n_reads, 1), np.uint32)
        self.counters = np.zeros(max(self.n_reads, 1), mb.COUNTER_DTYPE)
        self._c = mb.BatchResultC(n_reads=self.n_reads, n_hits=self.n_hits, n_ops=self.n_ops, hit_begin=self.hit_begin.ctypes.data,
                                  hits=self.hits_arr.ctypes.data if self.n_hits else None, ops=self.ops.ctypes.data if self.n_ops else None,
                                  status=self.status.ctypes.data, counters=self.counters.ctypes.data, d_arrays=None, n_second_pass=0, n_third_pass=0)
        self._cptr = C.pointer(self._c)

    @classmethod
    def from_lists(cls, lists, ops_of):
        """lists: per read, a structured array of hits (its ops_offset points into `ops_of`); the edit tracks are laid out again, contiguously, in read order"""
        hit_begin = np.concatenate([[0], np.cumsum([len(h) for h in lists])]).astype(np.uint64)
        hits = np.concatenate(lists) if any(len(h) for h in lists) else np.zeros(0, mb.HIT_DTYPE)
        ops = [ops_of[int(h["ops_offset"]):int(h["ops_offset"]) + int(h["n_ops"])] for h in hits]
        hits = hits.copy()
        n_ops = hits["n_ops"].astype(np.int64)
        hits["ops_offset"] = np.cumsum(n_ops) - n_ops
        return cls(hit_begin, hits, np.concatenate(ops) if ops else np.zeros(0, np.uint32))

    def lists(self):
        hb = self.hit_begin.astype(np.int64)
        return [self.hits_arr[hb[i]:hb[i + 1]] for i in range(self.n_reads)]

    def prefix(self, k):
        return CallerResult.from_lists(self.lists()[:k], self.ops)

    def edited(self, fn):
        """fn(read index, its hits) -> the hits that read keeps"""
        return CallerResult.from_lists([fn(i, h) for i, h in enumerate(self.lists())], self.ops)


def copy_of(res):
    """a caller-built copy of a result's own arrays"""
    return CallerResult(res.hit_begin.copy(), res.hits_arr.copy(), res.ops.copy())


def hit_lists_b(res):
    """Read i receives the hits of reads i, i + 1, ... (wrapping round) until it has list_lengths_b()[i]; every second read gets its scores tied in pairs, every fourth strictly descending ones, the rest
    keep theirs (exact matches all score 0: ties at the top); each list is sorted by descending score with a stable sort — such an array is a valid BinaryHeap."""
    n = res.n_reads
    hb = res.hit_begin.astype(np.int64)
    want = list_lengths_b(n)
    lists = []
    for i in range(n):
        got, j = [], i
        while sum(len(g) for g in got) < want[i] and j < i + n:
            got.append(res.hits_arr[hb[j % n]:hb[j % n + 1]])
            j += 1
        h = np.concatenate(got)[:want[i]].copy()
        h = h[np.argsort(-h["score"], kind="stable")]
        if i % 4 in (1, 2):
            h["score"][1::2] = h["score"][0:len(h) - len(h) % 2:2]  # (a, a, c, c, ...): still descending
        elif i % 4 == 0:
            h["score"] -= np.float32(0.125) * np.arange(len(h), dtype=np.float32)  # no ties at all (exact matches all score 0), and scores that end in .125 / .375 in XA
        lists.append(h)
    return CallerResult.from_lists(lists, res.ops)


PREFIXES_B = (1, 63, 64, 65, 129)  # reads: one lane, a wavefront less one, a full one, one more, two and one


def edge_batches_b(cres):
    """wavefronts (64 reads) that are entirely unmapped, a batch without any hit, and a mapped batch without a single (score, size) pair"""
    return {"first_64_without_hits": cres.edited(lambda i, h: h[:0] if i < 64 else h),
            "all_unmapped": cres.edited(lambda i, h: h[:0]),
            "no_second_hit": cres.edited(lambda i, h: h[:1])}


def pairs_needed(cres, recs):
    """The (score, size) pairs text_kernel writes, counted from the hit lists: per mapped read, its other hits that interval_cross_check does not take for the
    reported one (a lower bound where several hits tie with the reported one)."""
    total = 0
    for h, r in zip(cres.lists(), recs):
        if not r["mapped"] or len(h) < 2:
            continue
        fewest = len(h)
        for b in h[h["score"].view(np.uint32) == np.float32(r["as_score"]).view(np.uint32)]:  # the reported hit, or the hits tied with it: the fewest pairs any of them leaves
            cross = (h["size"] == b["size"]) & ((h["lower"] == b["lower"]) | (h["lower_rev"] == b["lower_rev"]))  # (true of b itself)
            fewest = min(fewest, len(h) - int(cross.sum()))
        total += fewest
    return total


def initial_pools(n):
    """mapad_amd.hip: run_record_kernels asks for a text pool of 24 bytes per read + 64 KiB and a pair pool of 2 * n + 4096 floats = n + 2048 pairs.  These are the
    requests: DevBuf::ensure allocates an eighth more plus 64 elements, and the kernel is given that capacity (about 100 792 bytes and 3 461 pairs at n = 1000).  The
    factor of two the overflow test asks for beyond these figures covers that slack too; a bound of 1x would not."""
    return 24 * n + 65536, n + 2048


def edge_counts_b(cres, recs):
    lens = np.diff(cres.hit_begin.astype(np.int64))
    tied = sum(len(np.unique(h["score"].view(np.uint32))) < len(h) for h in cres.lists())
    return dict(reads=cres.n_reads, mapped=int((recs["mapped"] != 0).sum()), lists_of_20=int((lens == 20).sum()), longest=int(lens.max()), tied_reads=int(tied),
                tied_at_the_top=sum(len(h) >= 2 and h["score"][0] == h["score"][1] for h in cres.lists()),
                text_bytes=int(recs["cigar_len"].sum() + recs["md_len"].sum() + recs["xa_len"].sum()))


def check_reach_b(c):
    # the host path yields 525 lists of 20, 750 reads with tied scores, 748 of them tied at the top, every read mapped
    assert c["lists_of_20"] >= 260 and c["longest"] == 20 and c["tied_reads"] >= 100 and c["tied_at_the_top"] >= 100 and c["mapped"] == c["reads"], c
