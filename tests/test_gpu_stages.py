"""The seven per-batch accumulator stages behind records_kernel — duplicate marking, damage score, damage profile, coverage, pileup, allele likelihoods and
genotype likelihoods — switched on together in one context (run with -m gpu on an MI355X): three batches at pipeline depth 2, the second converted twice, then
a batch with no reads.  Every stage's summary, cells and per-read outputs equal those of a context that ran that stage alone over the same batches, and those
of its host accumulator over the same fetched results and seeds; a batch counts once however often it is converted (the empty one for the duplicates only);
every reset zeroes its own stage and no other; allele mode 0 takes the genotypes with it.  A reference of two contigs of a few kb and batches of 70 to 300
reads: the module takes seconds."""
import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import synth

import damage_util as du
import pileup_util as pu
from kat_util import resolve_params
from parity_util import DAMAGE

pytestmark = pytest.mark.gpu

DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 99
TOTAL, SPLIT = 9_000, 4_001
LENGTHS = [SPLIT, TOTAL - SPLIT]
STAGES = ("dedup", "dscore", "damage", "coverage", "pileup", "allele", "genotype")  # in launch order
TIMES = ("accumulate_ms", "summary_ms", "kernel_ms", "mark_ms")
EMPTY = (np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64))  # map_batch accepts a batch with no reads


def seed_at(first_read):
    return int(mapad_amd.lib().mapad_records_seed_at(SEED, first_read))


def canon(x, drop=TIMES):
    """a read-out as plain Python, its times left out: what == compares"""
    if isinstance(x, dict):
        return {k: canon(v, drop) for k, v in x.items() if k not in drop}
    if isinstance(x, (list, tuple)):
        return [canon(v, drop) for v in x]
    return x.tolist() if isinstance(x, np.ndarray) else x


def batches_of(g):
    """three batches of 270, 160 and 76 reads: synthetic reads with indels, copies of some of them (duplicates), reads from the repeat, reads on the contigs' ends"""
    edges = pu.hand_made([g[0:40], g[SPLIT:SPLIT + 40], g[SPLIT - 40:SPLIT], g[TOTAL - 40:TOTAL], synth.revcomp(g[SPLIT - 45:SPLIT]), synth.revcomp(g[TOTAL - 65:TOTAL])])
    out = []
    for k, (n, copies) in enumerate(((200, 50), (120, 24), (50, 10))):
        drawn = pu.concat(synth.reads(g, n, seed=5 + 10 * k, qual_range=(2, 40), damage=DMG, len_range=(20, 140), indel_frac=0.3),
                          synth.reads(g[2_000:2_200], n // 10, 45, seed=6 + 10 * k, exo_frac=0.0, damage=DMG), edges)
        out.append(du.with_duplicates(drawn, copies, seed=7 + 10 * k))
    return out


def switch_on(ctx, stages):
    ctx.set_pipeline_depth(2)
    if "dedup" in stages:
        ctx.set_mark_duplicates(1)
    if "dscore" in stages:
        ctx.set_damage_score(1)
    if "damage" in stages:
        ctx.set_damage_profile(1)
    if "coverage" in stages:
        ctx.set_coverage(1)
    if "pileup" in stages:
        ctx.set_pileup(1)
    if "allele" in stages or "genotype" in stages:  # (the genotype likelihoods ride on the allele likelihoods)
        ctx.set_allele_likelihoods(1)
    if "genotype" in stages:
        ctx.set_genotype_likelihoods(True)


def device_reading(ctx, stage):
    """(summary, cells) of one stage of a context, whether it is on or not"""
    windows = lambda f: [f(t, 0, n) for t, n in enumerate(LENGTHS)]  # noqa: E731
    return canon({"dedup": lambda: (ctx.duplicates(), None),
                  "dscore": lambda: (ctx.damage_scores(), None),
                  "damage": lambda: (ctx.damage_profile(), None),
                  "coverage": lambda: (ctx.coverage(), windows(ctx.coverage_depth)),
                  "pileup": lambda: (ctx.pileup(), windows(ctx.pileup_counts)),
                  "allele": lambda: (ctx.allele_summary(), windows(ctx.allele_cells)),
                  "genotype": lambda: (ctx.genotype_summary(), windows(ctx.genotype_cells))}[stage]())


class Hosts:
    """the host accumulators of all seven stages, fed the same fetched results"""

    def __init__(self, idx, params):
        self.idx, self.params = idx, params
        self.dedup, self.coverage, self.pileup, self.allele = mb.DedupHost(), mb.CoverageHost(idx, 1), mb.PileupHost(idx, 1), mb.AlleleHost(idx, 1, genotypes=True)
        self.dscore = self.damage = None
        self.per_read = []

    def add(self, res, batch, seed):
        flags = self.dedup.add(self.idx, self.params, res, seed=seed)
        score_q, scored, self.dscore = mb.damage_score_host(self.idx, self.params, res, *batch, seed=seed, into=self.dscore)
        self.damage = mb.damage_profile_host(self.idx, self.params, res, batch[0], batch[2], seed=seed, into=self.damage)
        self.coverage.add(self.params, res, seed=seed)
        self.pileup.add(self.params, res, *batch, seed=seed)
        self.allele.add(self.params, res, *batch, seed=seed)
        self.per_read.append(canon((flags, score_q, scored)))

    def reading(self, stage):
        windows = lambda f: [f(t, 0, n) for t, n in enumerate(LENGTHS)]  # noqa: E731
        return canon({"dedup": lambda: (self.dedup.summary(), None),
                      "dscore": lambda: (self.dscore, None),
                      "damage": lambda: (self.damage, None),
                      "coverage": lambda: (self.coverage.summary(), windows(self.coverage.depth)),
                      "pileup": lambda: (self.pileup.summary(), windows(self.pileup.counts)),
                      "allele": lambda: (self.allele.summary(), windows(self.allele.cells)),
                      "genotype": lambda: (self.allele.genotype_summary(), windows(self.allele.genotype_cells))}[stage]())


def run(ctx, batches, hosts=None):
    """The batches through ctx at depth 2, converted in order, the second one twice; then the empty batch.  -> per batch (duplicate flags, score_q, scored), the
    latter two None while the damage score is off"""
    per_read, flying, todo, first, k = [], [], list(batches), 0, 0
    while todo or flying:
        while todo and len(flying) < 2:
            ctx.submit_batch(*todo[0])
            flying.append(todo.pop(0))
        ctx.select_batch(len(flying) - 1)  # the oldest: batches are converted in order
        b = flying.pop(0)
        res = ctx.fetch()
        out = ctx.hits_to_records(res, *b, seed=seed_at(first), as_arrays=True)
        if k == 1:  # converted twice: the same records, flags and scores; no counter moves
            again = ctx.hits_to_records(res, *b, seed=seed_at(first), as_arrays=True)
            assert np.array_equal(again[0]["flags"], out[0]["flags"]) and all(np.array_equal(x, y) for x, y in zip(again[2:], out[2:]))
        flags = ((out[0]["flags"] & 0x400) != 0).astype(np.uint8)
        per_read.append(canon((flags,) + (tuple(out[2:]) if len(out) == 4 else (None, None))))
        if hosts is not None:
            hosts.add(res, b, seed_at(first))
        first += len(b[2]) - 1
        k += 1
    res = ctx.map_batch(*EMPTY)
    assert len(ctx.hits_to_records(res, *EMPTY, seed=seed_at(first), as_arrays=True)[0]) == 0
    if hosts is not None:
        hosts.add(res, EMPTY, seed_at(first))
    return per_read


@pytest.fixture(scope="module")
def world():
    g = synth.genome(TOTAL, seed=83)
    g[7_000:7_200] = g[2_000:2_200]  # a repeat: reads from it take the coordinate the seeded draw gives them
    idx = mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batches = batches_of(g)
    assert all(64 <= len(b[2]) - 1 <= 300 for b in batches)
    ctx, hosts = mapad_amd.Context(idx, params, 0), Hosts(idx, params)
    switch_on(ctx, STAGES)
    per_read = run(ctx, batches, hosts)
    w = {"idx": idx, "params": params, "batches": batches, "ctx": ctx, "hosts": hosts, "per_read": per_read, "all": {s: device_reading(ctx, s) for s in STAGES}}
    yield w
    ctx.close()


@pytest.mark.parametrize("stage", STAGES)
def test_all_on_equals_the_stage_alone(world, stage):
    ctx = mapad_amd.Context(world["idx"], world["params"], 0)
    try:
        switch_on(ctx, (stage,))
        per_read = run(ctx, world["batches"])
        assert device_reading(ctx, stage) == world["all"][stage]
        for other in STAGES:  # and alone is alone
            if other != stage and (other, stage) != ("allele", "genotype"):
                assert device_reading(ctx, other)[0].get("batches", 0) == 0, other
    finally:
        ctx.close()
    col = {"dedup": 0, "dscore": slice(1, 3)}.get(stage)
    if col is not None:
        assert [p[col] for p in per_read] == [p[col] for p in world["per_read"]]


@pytest.mark.parametrize("stage", STAGES)
def test_all_on_equals_the_host_accumulators(world, stage):
    got, want = world["all"][stage], world["hosts"].reading(stage)
    if stage == "dedup":  # (the host's table is a table of its own: its size and its growth are not the device's)
        got, want = canon(got, ("slots", "grows")), canon(want, ("slots", "grows"))
    assert got == want
    assert world["per_read"] == world["hosts"].per_read[:3]


def test_a_batch_counts_once_and_something_was_counted(world):
    n = sum(len(b[2]) - 1 for b in world["batches"])
    batches = {s: world["all"][s][0]["batches"] for s in STAGES}
    assert batches == dict({s: 3 for s in STAGES}, dedup=4)  # the empty batch counts for the duplicates only
    a = {s: world["all"][s][0] for s in STAGES}
    assert a["dedup"]["reads_seen"] == a["dscore"]["reads_seen"] == a["damage"]["reads_seen"] == a["coverage"]["reads_seen"] == a["pileup"]["reads_seen"] == a["allele"]["reads_seen"] == n
    assert a["dedup"]["duplicates"] > 0 and a["dscore"]["reads_scored"] > 0 and a["damage"]["reads"] > 0 and a["coverage"]["covered_columns"] > 0
    assert a["pileup"]["columns_counted"] > 0 and a["allele"]["columns_counted"] > 0 and a["genotype"]["on"] == 1
    assert all(any(any(row) for row in cells) for cells in world["all"]["genotype"][1])
    assert sum(sum(f) for f, _, _ in world["per_read"]) == a["dedup"]["duplicates"]


def test_every_reset_zeroes_its_own_stage_and_allele_mode_0_takes_the_genotypes(world):
    """(last in the module: it empties the shared context)"""
    ctx = world["ctx"]
    resets = {"dedup": ctx.duplicates_reset, "dscore": ctx.reset_damage_scores, "damage": ctx.reset_damage_profile, "coverage": ctx.reset_coverage,
              "pileup": ctx.pileup_reset, "allele": ctx.allele_reset}
    live = set(STAGES)
    assert {s: device_reading(ctx, s) for s in STAGES} == world["all"]
    for stage, reset in resets.items():
        reset()
        live -= {stage, "genotype"} if stage == "allele" else {stage}  # the het cells describe the allele cells' columns: they go together
        for s in STAGES:
            summary, cells = device_reading(ctx, s)
            if s in live:
                assert [summary, cells] == world["all"][s], (stage, s)
                continue
            assert summary["batches"] == 0 and summary.get("reads_seen", 0) == 0, (stage, s)
            assert not any(np.asarray(summary[k]).any() for k in ("counts", "histogram") if k in summary), (stage, s)
            assert cells is None or not np.concatenate([np.asarray(x).ravel() for c in cells for x in (c if s == "allele" else [c])]).any(), (stage, s)
    assert ctx.duplicates()["slots"] == world["all"]["dedup"][0]["slots"]  # the table keeps its size
    assert ctx.genotype_summary()["on"] == 1 and ctx.allele_summary()["mode"] == 1
    ctx.set_allele_likelihoods(0)
    assert ctx.genotype_summary()["on"] == 0 and ctx.allele_summary()["mode"] == 0
