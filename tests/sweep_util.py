"""Input builders and case tables of the search parity sweeps (tests/test_gpu_sweeps.py on the GPU, tests/test_sweeps_host.py through the host build of the
kernels' per-read logic): one table, two runners, so the CPU twin and the GPU test cannot drift apart.

A. parameter grid: the user-facing search parameters the presets never vary (gap distance from the ends, number of gaps, gap penalties, -p, -D, asymmetric damage)
B. length ladders: every read length from 1 to 130 in one batch, and small batches around the read lengths at which a launch changes its memory layout
C. structured reference: tandem repeats, a homopolymer, short-period repeats, an X run and contig joins instead of an i.i.d. genome

Every case is compared word for word with the CPU oracle (parity_util.assert_same_as_oracle) and carries a reach-condition on the ORACLE's result, so that a case
cannot pass without meeting what it is for."""
import numpy as np

import mapad_amd
from mapad_amd import synth
from oracle import binding as ob

from kat_util import resolve_params
from parity_util import CONTINUOUS, DAMAGE, DOUBLE_STRANDED, IGNORE_BQ, NO_DAMAGE, VINDIJA, oracle_threads, split_reads

_DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)


class World:
    """One reference text: the product's index, the oracle's index over the same BWT, and the oracle's results by case (computed once, shared, never modified)."""

    def __init__(self, contigs):
        self.contigs = contigs
        self.pidx = mapad_amd.Index.build(contigs)
        self.oidx = ob.OracleIndex.from_bwt(self.pidx.bwt(), "$ACGTX", 128)
        self.n = sum(len(c[1]) for c in contigs)  # the forward strand's length: the index holds text $ revcomp $
        self._ores = {}

    def oracle(self, key, rp, batch):
        if key not in self._ores:
            reads, qs = split_reads(*batch)
            self._ores[key] = self.oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=min(8, oracle_threads()), keep_d=True)
        return self._ores[key]

    def anchors(self, interval):
        """Forward-strand coordinate of one base of each occurrence of a hit interval: the alignment's first base on the forward strand, its last base on the other."""
        lower, _, size = (int(x) for x in interval)
        p = self.pidx.sa_get_batch(np.arange(lower, lower + size, dtype=np.uint64)).astype(np.int64)
        return np.where(p < self.n, p, 2 * self.n - p)  # text $ revcomp $: row value n + 1 + q is forward base n - 1 - q


def pack(reads, quals):
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate([np.asarray(r, np.uint8) for r in reads]), np.concatenate([np.asarray(q, np.uint8) for q in quals]), offsets


def gapped_hits(ores):
    """per oracle hit: does its edit track hold an insertion or a deletion (oracle/binding.py: OP_KINDS, kind in the top byte)"""
    is_gap = np.concatenate([[0], np.cumsum((ores.ops >> 24) <= 1)])
    return np.diff(is_gap[ores.op_offsets.astype(np.int64)]) > 0


def hits_per_read(ores):
    return np.diff(ores.hit_offsets.astype(np.int64))


# ---- A. parameter grid --------------------------------------------------------------------------------------------------------------------------------------
GRID_GENOME = dict(n_bp=200_000, seed=61)


def grid_world():
    """the world of parts A and B with its genome and the grid's read batch"""
    w = World([("chr1", synth.genome(**GRID_GENOME))])
    w.genome = w.contigs[0][1]
    w.grid_batch = grid_reads(w.genome)
    return w


def struct_worlds():
    return {multi: structured_world(multi) for multi in (False, True)}


def grid_reads(g):
    """35-70 bp, damaged, a tenth of the endogenous reads with a 1-2 base indel; 30 is more than half of every read"""
    return synth.reads(g, 300, 50, seed=31, qual_range=(20, 40), damage=_DMG, len_range=(35, 70), indel_frac=0.1)


# the cheaper gap: -i 0.05 instead of 0.001 (-4.3 instead of -10.0 to open) and half a representative mismatch per extended base (-3.6 instead of -7.2).  Chosen on the CPU: the oracle's longest search of
# grid_reads stays below 2^17 pops (the idle hand-over threshold of the host tail), so the case tests the GPU search and not the host tail.  (-4 / -1 makes the
# searches of these reads explode to the reference's limits: EXPLOSIVE_GAP below.)
CHEAPER_GAP = dict(penalty_gap_open={"log2": 0.05}, penalty_gap_extend={"repr_mm_times": 0.5})
GRID_MAX_POPS = 1 << 17

# (id, preset, overrides, do the parameters allow a gap in a read of grid_reads)
GRID_CASES = [
    ("gde0", DAMAGE, dict(gap_dist_ends=0), True),
    ("gde1", DAMAGE, dict(gap_dist_ends=1), True),
    ("gde30", DAMAGE, dict(gap_dist_ends=30), False),
    ("gaps0", DAMAGE, dict(max_num_gaps_open=0), False),
    ("gaps1", DAMAGE, dict(max_num_gaps_open=1), True),
    ("gaps3", DAMAGE, dict(max_num_gaps_open=3), True),
    ("p0.01", DAMAGE, dict(poisson_threshold=0.01), True),
    ("p0.1", DAMAGE, dict(poisson_threshold=0.1), True),
    ("D0.03", DAMAGE, dict(divergence={"div3": 0.03}), True),  # `-D 0.03` as the command line derives it
    ("divergence0.03", DAMAGE, dict(divergence=0.03), True),  # the parameter itself at 0.03
    ("asym_damage", DAMAGE, dict(five_prime_overhang=0.3, three_prime_overhang=0.7, ds_deamination_rate=0.05, ss_deamination_rate=0.6), True),
    ("cheaper_gap", DAMAGE, CHEAPER_GAP, True),
    # (with the presets' gap penalties a second open gap is never within the bound, so 1, 2 and 3 search alike; with the cheaper gap they do not)
    ("cheaper_gap_gaps1", DAMAGE, dict(CHEAPER_GAP, max_num_gaps_open=1), True),
    ("cheaper_gap_gaps3", DAMAGE, dict(CHEAPER_GAP, max_num_gaps_open=3), True),
    ("continuous_gde0", CONTINUOUS, dict(gap_dist_ends=0), True),
    ("continuous_c0.25_e1.1", CONTINUOUS, dict(cutoff=-0.25, exponent=1.1), True),
    ("double_stranded_gaps1", DOUBLE_STRANDED, dict(max_num_gaps_open=1), True),
    ("ignore_bq_gde0", IGNORE_BQ, dict(gap_dist_ends=0), True),
    ("vindija_gde0_gaps1", VINDIJA, dict(gap_dist_ends=0, max_num_gaps_open=1), True),
]
GRID_IDS = [c[0] for c in GRID_CASES]
# the launch variants of the grid (GPU only): (case id, environment)
GRID_LAUNCH_VARIANTS = [(cid, {"MAPAD_LANES_PER_READ": lpr}) for cid in ("gde0", "gaps0") for lpr in ("2", "1")] + [("gde0", {"MAPAD_GENERAL_DIRECTION": "1"})]


def grid_case(cid):
    _, preset, over, gaps = GRID_CASES[GRID_IDS.index(cid)]
    return resolve_params(dict(preset, **over)), gaps


def check_grid_reach(cid, ores):
    _, gaps = grid_case(cid)
    g = gapped_hits(ores)
    assert g.any() == gaps, f"{cid}: {int(g.sum())} oracle hits with a gapped edit track"
    assert hits_per_read(ores).astype(bool).sum() > 100  # most endogenous reads map
    assert int(ores.counters[:, 3].max()) < GRID_MAX_POPS


# The lead behind CHEAPER_GAP: DAMAGE with gaps at -4 / -1 and the reference's own limits (2 M heap entries, 10 M edit-tree nodes).  The searches of grid_reads
# explode (oracle: 830 K pops per read on average, seven reads end at the 10 M limit).  Read 30 of the batch is the cheapest of the 24 whose edit trees outgrow
# 2^22 nodes: 58 bases, 2.9 M pops, 6.0 M nodes.
EXPLOSIVE_GAP = dict(penalty_gap_open=-4.0, penalty_gap_extend=-1.0)
EXPLOSIVE_READ = 30


def explosive_case(world):
    reads, qs = split_reads(*world.grid_batch)
    return resolve_params(dict(DAMAGE, **EXPLOSIVE_GAP)), pack([np.frombuffer(reads[EXPLOSIVE_READ], np.uint8)], [qs[EXPLOSIVE_READ]])


def check_explosive_reach(ores):
    assert int(ores.counters[0, 4]) > 1 << 22 and int(ores.counters[0, 3]) > 1 << 21 and hits_per_read(ores)[0] > 0


# ---- B. length ladders --------------------------------------------------------------------------------------------------------------------------------------
def ladder_reads(g, lengths, seed):
    """Reads cut from the genome, each at its own length; two in three carry one substitution, every second one is reverse-complemented; qualities 20-40."""
    rng = np.random.default_rng(seed)
    reads = []
    for i, L in enumerate(lengths):
        pos = int(rng.integers(0, len(g) - L))
        s = g[pos:pos + L].copy()
        at = int(rng.integers(0, L))
        if i % 3 != 2:
            s[at] = ord("ACGT"[("ACGT".index(chr(s[at])) + 1 + int(rng.integers(0, 3))) % 4])
        reads.append(synth.revcomp(s) if i % 2 else s)
    return pack(reads, [rng.integers(20, 41, len(r)).astype(np.uint8) for r in reads])


B1_LENGTHS = list(range(1, 131))  # one score table per length; lengths 2-15 (offset chains longer than the part they scan), L / 2 == 0, L < 2 * gap_dist_ends, 17, 64, 128
# (under the continuous bound a 17- or 19-base read with a substitution maps only if the substitution is a cheap one; with this seed of ladder_reads the oracle
# maps every read of 17 bases and more under all four parameter sets)
B1_SEED = 1
B1_MODELS = [("damage", DAMAGE, {}), ("continuous", CONTINUOUS, {}), ("vindija", VINDIJA, {}), ("damage_gde0", DAMAGE, dict(gap_dist_ends=0))]
B1_IDS = [m[0] for m in B1_MODELS]


# a batch of short reads only, two of each length: the longest read is shorter than the longest offset chain of the D array (15 chains per part; the chains'
# buffers are sized by the batch's longest read)
B1_SHORT_ONLY = list(range(1, 15)) * 2


def b1_params(mid):
    _, preset, over = B1_MODELS[B1_IDS.index(mid)]
    return resolve_params(dict(preset, **over))


def layout_batch(g, lmax):
    """Six reads whose longest has exactly `lmax` bases — a launch picks its layout by the batch's longest read.  (The 100-base read of the longer batches
    would be the longest of the 85 | 86 ones: 60 there.)"""
    batch = ladder_reads(g, [lmax, lmax - 1, 50, 17, 100 if lmax > 100 else 60, lmax], seed=lmax)
    assert int(np.diff(batch[2].astype(np.int64)).max()) == lmax
    return batch


# The read lengths at which a launch changes its layout, written down (not derived from the library's constants: a changed threshold must show up here as a
# test someone has to look at):
#   85 | 86      single lanes: near data in LDS while near_bytes(lmax) * 64 <= 64 KiB        mapad_amd.hip: map_batch launch, `near_fits` (lanes-per-read 1)
#   256 | 257    quads: near data in LDS up to kMaxLdsReadLen = 256                          mapad_amd.hip: `constexpr uint32_t kMaxLdsReadLen = 256`
#   298 | 299    pairs: near data in LDS while near_bytes(lmax, top) * 32 <= 64 KiB          mapad_amd.hip: `near_fits` (lanes-per-read 2)
#   768 | 769    D-array chains in LDS while 16 * lmax * 4 bytes <= 48 KiB                   mapad_amd.hip: `if (lds_bytes > 48 * 1024)`
#   1024 | 1025  heavy wavefronts: position data in LDS up to kHeavyMaxLdsReadLen = 1024     heavy_kernel.hpp: `constexpr uint32_t kHeavyMaxLdsReadLen = 1024`
B1_SINGLE_LANE_LMAX = [85, 86]
B2_LMAX = [255, 256, 257, 298, 299, 300, 767, 768, 769, 1023, 1024, 1025]
B2_PAIRS_LMAX = [255, 256, 257, 298, 299, 300]
B2_HEAVY_LMAX = [1023, 1024, 1025]


def check_ladder_reach(ores, offsets):
    lens = np.diff(offsets.astype(np.int64))
    unmapped = lens[(hits_per_read(ores) == 0) & (lens >= 17)]
    assert unmapped.size == 0, f"reads of {unmapped.tolist()} bases do not map"


# ---- C. structured reference --------------------------------------------------------------------------------------------------------------------------------
def structured_text():
    """-> (text, regions): 20 kbp uniform | 12 tandem copies of a 500 bp unit | A x 300 | ACGTTGCA x 60 | CA x 200 | the unit's reverse complement | 20 kbp uniform"""
    unit = synth.genome(500, seed=71)
    parts = [("flank5", synth.genome(20_000, seed=72)), ("tandem", np.tile(unit, 12)), ("homopolymer", np.full(300, ord("A"), np.uint8)),
             ("period8", np.tile(np.frombuffer(b"ACGTTGCA", np.uint8), 60)), ("period2", np.tile(np.frombuffer(b"CA", np.uint8), 200)), ("unit_rc", synth.revcomp(unit)),
             ("flank3", synth.genome(20_000, seed=73))]
    regions, at = {}, 0
    for name, a in parts:
        regions[name] = (at, at + len(a))
        at += len(a)
    return np.concatenate([a for _, a in parts]), regions


N_RUN = (10_000, 10_030)  # 30 N: long enough to stay an X run in the index (runs of 20 and more do)
JOINS = (23_000, 27_100)  # inside the tandem array, inside the period-8 stretch


def structured_world(multi):
    text, regions = structured_text()
    if not multi:
        return World([("chr1", text)]), text, regions
    t = text.copy()
    t[N_RUN[0]:N_RUN[1]] = ord("N")
    return World([("one", t[:JOINS[0]]), ("two", t[JOINS[0]:JOINS[1]]), ("three", t[JOINS[1]:])]), t, regions


def structured_reads(text, regions, qual_range, hand_laid):
    """300 reads of 30-70 bp from the structured stretch and a kilobase of either flank, none exogenous, a tenth with an indel; `hand_laid`: plus reads across the
    N run (bases N in the read, an X run in the index), beside it, and across the two contig joins"""
    lo, hi = regions["tandem"][0] - 1000, regions["unit_rc"][1] + 1000
    kw = dict(qual=40) if qual_range is None else dict(qual_range=qual_range)
    seqs, quals, offsets = synth.reads(text[lo:hi], 300, 50, seed=83, exo_frac=0.0, len_range=(30, 70), indel_frac=0.1, **kw)
    if not hand_laid:
        return seqs, quals, offsets
    a, b = N_RUN
    cuts = [(a - 25, b + 25), (a - 48, a + 2), (b - 2, b + 48), (a - 40, a), (b, b + 40), (a - 30, a + 20)]  # through the run, two bases into it, flush against it
    cuts += [(j - 25, j + 25) for j in JOINS] + [(JOINS[0] - 5, JOINS[0] + 55), (JOINS[1] - 60, JOINS[1] + 3)]
    extra = [text[s:e].copy() for s, e in cuts]
    extra.append(np.concatenate([text[a - 25:a], text[b:b + 25]]))  # the run cut out of the read
    extra.append(synth.revcomp(text[a - 45:a + 3]))
    extra.append(synth.revcomp(text[JOINS[0] - 30:JOINS[0] + 30]))
    rng = np.random.default_rng(5)
    reads, qs = split_reads(seqs, quals, offsets)
    reads = [np.frombuffer(r, np.uint8) for r in reads] + extra
    qs = list(qs) + [np.full(len(e), 40, np.uint8) if qual_range is None else rng.integers(qual_range[0], qual_range[1] + 1, len(e)).astype(np.uint8) for e in extra]
    return pack(reads, qs)


# (id, several contigs with an N run and hand-laid reads, preset, quality range of the reads — None: q40 throughout, for ties in the heap order)
STRUCT_CASES = [("one_contig_damage", False, DAMAGE, (20, 40)), ("one_contig_no_damage_q40", False, NO_DAMAGE, None),
                ("three_contigs_damage", True, DAMAGE, (20, 40)), ("three_contigs_no_damage_q40", True, NO_DAMAGE, None)]
STRUCT_IDS = [c[0] for c in STRUCT_CASES]
# the launch variants (GPU only): many hits per read through the retry of an overflowing hit pool; base arenas of 32 nodes
STRUCT_LAUNCH_VARIANTS = [("one_contig_damage", {"MAPAD_HIT_POOL": "64"}), ("three_contigs_no_damage_q40", {"MAPAD_TIER0_NODES": "32"})]


def struct_case(cid, worlds):
    """worlds: {multi: structured_world(multi)} -> (world, params, batch)"""
    _, multi, preset, qr = STRUCT_CASES[STRUCT_IDS.index(cid)]
    world, text, regions = worlds[multi]
    return world, resolve_params(preset), structured_reads(text, regions, qr, hand_laid=multi)


def check_struct_reach(cid, world, regions, ores):
    assert int((ores.intervals[:, 2] >= 5).sum()) > 50, "hit intervals of many rows"
    inside = {"homopolymer": 0, "period2": 0}
    for r in np.flatnonzero(hits_per_read(ores)):
        h0, h1 = int(ores.hit_offsets[r]), int(ores.hit_offsets[r + 1])
        best = h0 + int(np.argmax(ores.scores[h0:h1]))
        at = world.anchors(ores.intervals[best])
        for name in inside:
            lo, hi = regions[name]
            inside[name] += bool(((at >= lo) & (at < hi)).all())
    assert inside["homopolymer"] >= 1 and inside["period2"] >= 1, f"{cid}: reads with their best hit inside {inside}"
