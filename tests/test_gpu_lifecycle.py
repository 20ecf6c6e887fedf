"""The release and re-allocate paths of the device buffers and events (run with -m gpu on an MI355X).  One context at pipeline depth 3 with all nine accumulator
stages on maps a batch, converts it and reads every stage out; then every stage is switched off and on again (each setter's release path, each buffer's
allocation) and the same batch goes through again; then the depth goes to 1 and to 2 (the batch slots give their memory back) and it goes through once more;
then the context is destroyed, a new one is made on the same index and it goes through a last time.  Every read-out, times left out, the records and every
fetched hit array equal those of the first round, and those of a fresh context that has one stage on.  The reference and the batch are those of
tests/test_gpu_stages.py, its first batch of 276 reads over 9 000 bp: the module takes seconds."""
import numpy as np
import pytest

import mapad_amd
from mapad_amd import synth

import panel_util as pn
import test_gpu_stages as gs
from test_gpu_stages import SEED, SPLIT, TOTAL, canon
from kat_util import resolve_params
from parity_util import DAMAGE

pytestmark = pytest.mark.gpu

STAGES = ("dedup", "dscore", "rescale", "damage", "coverage", "pileup", "allele", "genotype", "panel")  # in launch order


def panel_of(g):
    """a row on every 37th base, the contigs' first and last bases among them: the reference's base against the next one in ACGT"""
    x = np.unique(np.concatenate([np.arange(0, TOTAL, 37), [SPLIT - 1, SPLIT, TOTAL - 1]]))
    tid = (x >= SPLIT).astype(np.int32)
    return tid, (x - tid * SPLIT).astype(np.uint64), g[x].copy(), pn._next(g[x])


def switch(ctx, stages, panel, on=True):
    """the stages on (mode 1) or off (mode 0, which frees what the stage holds); the genotype likelihoods ride on the allele likelihoods"""
    if "dedup" in stages:
        ctx.set_mark_duplicates(int(on))
    if "dscore" in stages:
        ctx.set_damage_score(int(on))
    if "rescale" in stages:
        ctx.set_quality_rescale(int(on))
    if "damage" in stages:
        ctx.set_damage_profile(int(on))
    if "coverage" in stages:
        ctx.set_coverage(int(on))
    if "pileup" in stages:
        ctx.set_pileup(int(on))
    if "genotype" in stages and not on:
        ctx.set_genotype_likelihoods(False)
    if "allele" in stages or "genotype" in stages:
        ctx.set_allele_likelihoods(int(on))
    if "genotype" in stages and on:
        ctx.set_genotype_likelihoods(True)
    if "panel" in stages:
        ctx.set_snp_panel(1, *panel) if on else ctx.set_snp_panel(0)


def reset_all(ctx):
    for reset in (ctx.duplicates_reset, ctx.reset_damage_scores, ctx.reset_quality_rescale, ctx.reset_damage_profile, ctx.reset_coverage, ctx.pileup_reset,
                  ctx.allele_reset, ctx.snp_panel_reset):
        reset()


def reading(ctx, stage, n_rows):
    if stage == "rescale":
        return canon((ctx.quality_rescale(), None))
    if stage == "panel":
        return canon((ctx.snp_panel(), (ctx.snp_panel_counts(0, n_rows), ctx.snp_panel_calls(0, n_rows))))
    return gs.device_reading(ctx, stage)


def one_round(ctx, batch, stages, n_rows):
    """the batch mapped and converted -> (the fetched hit arrays, the records and what travels with them, every stage's read-out)"""
    res = ctx.map_batch(*batch)
    hits = canon((res.hit_begin, res.hits_arr, res.ops, res.status))
    recs, rescaled = ctx.hits_to_records(res, *batch, seed=SEED, rescaled=True)
    records = ([sorted((k, repr(v)) for k, v in r.items()) for r in recs], None if rescaled is None else rescaled.tolist())  # (decoded: the fields' places in the text pool are not part of a record)
    return hits, records, {s: reading(ctx, s, n_rows) for s in stages}


@pytest.fixture(scope="module")
def world():
    g = synth.genome(TOTAL, seed=83)
    g[7_000:7_200] = g[2_000:2_200]
    idx = mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = gs.batches_of(g)[0]
    assert len(batch[2]) - 1 == 276  # 200 drawn, 20 from the repeat, 6 on the contigs' ends, 50 copies
    panel = panel_of(g)
    n_rows = len(panel[0])
    rounds = []
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_pipeline_depth(3)
        switch(ctx, STAGES, panel)
        rounds.append(one_round(ctx, batch, STAGES, n_rows))
        switch(ctx, STAGES, panel, on=False)  # every setter's release path ...
        switch(ctx, STAGES, panel)            # ... and every allocation again
        rounds.append(one_round(ctx, batch, STAGES, n_rows))
        ctx.set_pipeline_depth(1)  # the slots beyond the first give their memory and events back
        ctx.set_pipeline_depth(2)
        reset_all(ctx)
        rounds.append(one_round(ctx, batch, STAGES, n_rows))
    finally:
        ctx.close()
    ctx = mapad_amd.Context(idx, params, 0)  # a new context on the same index
    try:
        ctx.set_pipeline_depth(3)
        switch(ctx, STAGES, panel)
        rounds.append(one_round(ctx, batch, STAGES, n_rows))
    finally:
        ctx.close()
    return {"idx": idx, "params": params, "batch": batch, "panel": panel, "n_rows": n_rows, "rounds": rounds}


@pytest.mark.parametrize("k, what", [(1, "every stage off and on again"), (2, "depth 1, then 2"), (3, "a new context")])
def test_a_later_round_equals_the_first(world, k, what):
    first, later = world["rounds"][0], world["rounds"][k]
    assert later[0] == first[0], what
    assert later[1] == first[1], what
    for s in STAGES:
        assert later[2][s] == first[2][s], (what, s)


@pytest.mark.parametrize("stage", STAGES)
def test_the_first_round_equals_a_context_with_one_stage(world, stage):
    ctx = mapad_amd.Context(world["idx"], world["params"], 0)
    try:
        switch(ctx, (stage,), world["panel"])
        hits, _, got = one_round(ctx, world["batch"], (stage,), world["n_rows"])
    finally:
        ctx.close()
    assert hits == world["rounds"][0][0]
    assert got[stage] == world["rounds"][0][2][stage]


def test_something_was_counted(world):
    hits, records, read = world["rounds"][0]
    assert len(hits[1]) > 200 and len(records[0]) == 276 and len(records[1]) == int(world["batch"][2][-1])
    assert sum(("damage_score", "None") not in r for r in records[0]) > 100 and sum(("duplicate", "True") in r for r in records[0]) > 0
    a = {s: read[s][0] for s in STAGES}
    assert all(a[s]["batches"] == 1 for s in STAGES) and a["genotype"]["on"] == 1
    assert a["dedup"]["duplicates"] > 0 and a["dscore"]["reads_scored"] > 0 and a["rescale"]["bases_changed"] > 0 and a["damage"]["reads"] > 0
    assert a["coverage"]["covered_columns"] > 0 and a["pileup"]["columns_counted"] > 0 and a["allele"]["columns_counted"] > 0 and a["panel"]["reads_on_panel"] > 0
    assert np.asarray(read["panel"][1][0]).any() and all(any(any(row) for row in cells) for cells in read["genotype"][1])
