"""Search parity over the whole base-quality byte and the whole read alphabet on the GPU (run with -m gpu on an MI355X): the cases of tests/quality_util.py — one or
two bases at Q0 / Q1, where the model's optimal symbol is a mismatch; N at Q0 / Q2; every byte a read file can hold in place of a base; qualities 41-93, 255 and
uniform over the byte; a ladder of per-read quality centres whose lowest rungs take millions of pops — through the HIP search and D-array kernels word for word
against the CPU oracle, through the record kernels field by field against the oracle's intervals_to_record, through the accumulator kernels against their independent
restatements, and through `mapad-amd map`.  tests/test_quality_host.py runs the same table through the host build of the per-read logic and the host paths."""
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb

import allele_util as au
import cli_audit_util as au_cli
import dscore_util as ds
import genotype_util as gu
import pileup_util as pu
import quality_util as qu
import records_util as ru
import sweep_util as su
from bam_util import read_bam
from parity_util import assert_same_as_oracle

pytestmark = pytest.mark.gpu

world = pytest.fixture(scope="module")(su.grid_world)
TEXT_MODES = ["device", "host"]  # MAPAD_RECORDS_TEXT
_TAIL_SWITCHES = ("MAPAD_TAIL_BACKLOG_BUDGET", "MAPAD_TAIL_BACKLOG_IDLE", "MAPAD_TAIL_BACKLOG", "MAPAD_TAIL_POPS_IDLE", "MAPAD_TAIL_MIN_CLASS", "MAPAD_TAIL_CONTINUE",
                  "MAPAD_TAIL_RING", "MAPAD_TAIL_THREADS", "MAPAD_TIER0_NODES", "MAPAD_CLASS_COUNTS")


def _gpu_map(world, preset, batch, tail_pops=None):
    ctx = mapad_amd.Context(world.pidx, mapad_amd.make_params(qu.params(preset)), 0)  # (the launch switches of the environment are read here)
    try:
        if tail_pops is not None:
            ctx.set_tail_pops(tail_pops)
        return ctx.map_batch(*batch), ctx.tail_info()
    finally:
        ctx.close()


def _env_id(cid, preset, env):
    return f"{cid}-{preset}" + ("-" + ",".join(f"{k[6:].lower()}={v}" for k, v in env.items()) if env else "")


# ---- search and D array -----------------------------------------------------------------------------------------------------------------------------------------
_CELLS = [(cid, preset, {}) for cid, preset in qu.CELLS] + qu.LAUNCH_VARIANTS


@pytest.mark.parametrize("cid,preset,env", _CELLS, ids=[_env_id(*c) for c in _CELLS])
def test_quality_and_alphabet_cases(world, cid, preset, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    batch = qu.case_batch(world, cid)
    ores = qu.oracle(world, cid, preset)
    qu.check_reach(cid, preset, ores, batch)
    if preset in qu.QUALITY_BLIND:
        qu.check_quality_blind(world, cid, preset)
    assert_same_as_oracle(ores, _gpu_map(world, preset, batch)[0], batch[2])


def test_quality_ladder_with_the_host_tail_at_its_shipped_settings(world, monkeypatch):
    """Per-read quality centres from 0 to 255 under DAMAGE, no tail switch set: the reads at Q0-Q5 pass 2^17 pops and leave for the host (asserted from tail_info());
    the whole batch equals the oracle's.  Then the reads below 2^17 pops with the tail off: the GPU search alone."""
    for v in _TAIL_SWITCHES:
        monkeypatch.delenv(v, raising=False)
    batch = qu.ladder_batch(world)
    ores = qu.ladder_oracle(world)
    counts, light = qu.check_ladder_reach(ores, batch)
    res, info = _gpu_map(world, "damage", batch)
    print("ladder", counts, info)
    assert info["reads"] >= 1, info
    assert_same_as_oracle(ores, res, batch[2])
    assert (res.status & 16).sum() == 0
    sub = qu.subset(batch, light)
    osub = world.oracle(("quality", "ladder", "below_2^17"), qu.params("damage"), sub)
    assert int(osub.counters[:, 3].max()) < su.GRID_MAX_POPS and osub.n == len(light) >= 250
    res, info = _gpu_map(world, "damage", sub, tail_pops=0)
    assert info["reads"] == 0
    assert_same_as_oracle(osub, res, sub[2])


# ---- records ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def record_world(world):
    return qu.record_world(world)


@pytest.mark.parametrize("preset", list(ru.PRESETS))
@pytest.mark.parametrize("cid", qu.RECORD_CASES)
def test_device_built_records_equal_the_oracles(world, record_world, cid, preset, monkeypatch):
    """MAPQ takes its optimal scores from the base qualities (mapping.rs:570-590); MD and NM name the reference base under a read byte outside ACGT"""
    batch = qu.case_batch(world, cid)
    ctx = mapad_amd.Context(world.pidx, ru.params(preset), 0)
    try:
        res = ctx.map_batch(*batch)
        ocanon = record_world.oracle_canon(preset, res, batch)
        for text in TEXT_MODES:
            monkeypatch.setenv("MAPAD_RECORDS_TEXT", text)
            recs, rtext = ctx.hits_to_records(res, *batch, seed=ru.SEED, as_arrays=True)
            n_bad, first, per_field = ru.differing((recs, rtext), ocanon)
            assert n_bad == 0, ru.report(first, per_field, f"{cid} {preset} {text}")
            qu.check_record_reach(cid, world.genome, recs, rtext, batch)
    finally:
        ctx.close()


# ---- accumulators -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", TEXT_MODES)
@pytest.mark.parametrize("name", qu.ACC_BATCHES)
def test_accumulators_at_the_ends_of_the_quality_axis(world, name, text, monkeypatch):
    """What dscore_kernel, allele_kernel, genotype_kernel and pileup_kernel make of qualities over the whole byte, at 255 throughout and in {0, 1, 254, 255}: equal
    to the host path and to the independent restatements (dscore_util, allele_util, genotype_util, pileup_util) over the device's own records, under either text path;
    the pileup with a quality floor of 0, 1 and 255 loses exactly the bases below it."""
    batch = qu.acc_batch(world, name)
    p = mapad_amd.make_params(qu.params("damage"))
    lengths = [len(world.genome)]
    monkeypatch.setenv("MAPAD_RECORDS_TEXT", text)
    ctx = mapad_amd.Context(world.pidx, p, 0)
    try:
        ctx.set_damage_score(1, 0.0)
        ctx.set_allele_likelihoods(1, 0, 0, 0)
        ctx.set_genotype_likelihoods(True)
        ctx.set_pileup(1, 0, 0, 0)
        res = ctx.map_batch(*batch)
        score_q, scored = ctx.hits_to_records(res, *batch, seed=qu.ACC_SEED, as_arrays=True)[2:]
        recs = ctx.hits_to_records(res, *batch, seed=qu.ACC_SEED)
        counted = qu.m_column_qualities(recs, batch)
        qu.check_accumulator_reach(name, counted)
        # the damage score
        want_q, want_scored, want = ds.from_records(p, recs, batch)
        assert np.array_equal(score_q, want_q) and np.array_equal(scored, want_scored) and (score_q != 0).any()
        ds.assert_summary(ctx.damage_scores(), want, name)
        hq, hs, hsum = mb.damage_score_host(world.pidx, p, res, *batch, seed=qu.ACC_SEED)
        assert np.array_equal(score_q, hq) and np.array_equal(scored, hs)
        ds.assert_summary(ctx.damage_scores(), hsum, name + ": host path")
        # allele and genotype likelihoods (the batch was counted once, however often it was converted)
        table = gu.from_records(p, lengths, recs, batch, 1)
        au.assert_equal(ctx.allele_summary(*qu.ACC_ALLELE_RULE), table, *qu.ACC_ALLELE_RULE, what=name, cells_of=ctx.allele_cells, consensus_of=ctx.allele_consensus)
        gu.assert_equal(ctx, table, qu.ACC_GENOTYPE_RULE, name)
        acc = mb.AlleleHost(world.pidx, 1, genotypes=True).add(p, res, *batch, seed=qu.ACC_SEED)
        au.assert_same_accumulators(au.ContextView(ctx), acc, lengths, [qu.ACC_ALLELE_RULE], name + ": host path")
        gu.assert_same(ctx, acc, lengths, [qu.ACC_GENOTYPE_RULE], name + ": host path")
        # the pileup under a quality floor (a change of the floor starts an empty table: the batch, still resident, counts into it)
        by_min_bq = {}
        for min_bq in qu.ACC_MIN_BQ:
            ctx.set_pileup(1, min_bq, 0, 0)
            ctx.hits_to_records(res, *batch, seed=qu.ACC_SEED, as_arrays=True)
            by_min_bq[min_bq] = ctx.pileup(*qu.ACC_PILEUP_RULE)
            pu.assert_equal(by_min_bq[min_bq], pu.from_records(lengths, recs, batch, 1, min_bq), *qu.ACC_PILEUP_RULE, what=f"{name}, min_bq {min_bq}",
                            counts_of=ctx.pileup_counts, consensus_of=ctx.pileup_consensus)
            pil = mb.PileupHost(world.pidx, 1, min_bq, 0, 0).add(p, res, *batch, seed=qu.ACC_SEED)
            pu.assert_equal(by_min_bq[min_bq], pil.summary(*qu.ACC_PILEUP_RULE), *qu.ACC_PILEUP_RULE, what=f"{name}, min_bq {min_bq}: host path")
        qu.check_low_quality_moves(name, by_min_bq, counted)
        with pytest.raises(mapad_amd.MapadError) as e:  # a floor no quality byte reaches is refused
            ctx.set_pileup(1, 256, 0, 0)
        assert e.value.code == -1
    finally:
        ctx.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------------
_died = []  # the first child that failed or ran into its time limit: no further one is started


def _child(cmd):
    if _died:
        pytest.fail(f"not started: an earlier child died ({_died[0]})")
    try:
        subprocess.check_call(["timeout", "-k", "10", "300"] + cmd)
    except subprocess.CalledProcessError as e:
        _died.append(f"exit status {e.returncode}: {' '.join(cmd[:4])} ...")
        raise


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    """the grid genome indexed on disk by `mapad-amd index`, and the two input files"""
    d = tmp_path_factory.mktemp("cli_quality")
    fa = str(d / "ref.fa")
    rworld = qu.cli_world(fa, _child)
    inputs = qu.cli_inputs(rworld.contigs[0][1])
    au_cli.check_cli_flags_are_the_preset(qu.CLI_PRESET)
    return dict(dir=str(d), fa=fa, world=rworld, inputs=inputs, files=qu.cli_write_inputs(str(d), inputs))


@pytest.mark.parametrize("form", ["fastq", "bam"])
def test_map_keeps_every_quality_byte(cli_run, form):
    """`mapad-amd map` over FASTQ quality strings that use every character from `!` to `~` | over BAM records of 0xFF at every position (records without
    qualities) and of raw qualities 94-254, every second one stored reversed: every written record equals the oracle's, and the written QUAL is the input's,
    reversed on reverse records.  Every run is one child process under a time limit of its own."""
    recs = cli_run["inputs"][form]
    rows, _ = qu.cli_expectation(cli_run["world"], recs)
    qu.check_cli_reach(rows)
    out = os.path.join(cli_run["dir"], form + ".out.bam")
    _child([au_cli.cli(), "--seed", str(qu.CLI_SEED), "map", "-r", cli_run["files"][form], "-g", cli_run["fa"], "-o", out, "--batch_size", "512"] + au_cli.cli_flags(qu.CLI_PRESET))  # (one chunk; the default reserves a context for 250 000 reads)
    _, refs, got = read_bam(out)
    assert refs == au_cli.header_refs(cli_run["world"])
    n_bad, first, per_field = au_cli.compare(got, rows, recs)
    assert n_bad == 0, au_cli.report(len(got), n_bad, first, per_field, form)
    for g, r in zip(got, recs):  # said once more, without the expectation: QUAL as it came in
        assert g["qual"] == (r["qual"][::-1] if g["flags"] & 0x10 else r["qual"]), r["name"]
