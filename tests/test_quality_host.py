"""CPU twin of tests/test_gpu_quality.py: the cases of tests/quality_util.py — base qualities over the whole byte, read bytes outside ACGT — through the host build
of the kernels' per-read logic (emu_util.map_batch) against the oracle, and their records through the host record path.  It validates the case table and its
reach-conditions without a GPU and protects the step code the kernels share (csrc/search_core.hpp, csrc/darray_core.hpp, csrc/common.hpp: base_index, sdm_row_at,
sdm_optimal).  What only exists on the device — the quad and pair commits, the D-array chains in LDS, the record and accumulator kernels — has no counterpart here."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from oracle import binding as ob

import allele_util as au
import cli_audit_util as au_cli
import dscore_util as ds
import emu_util
import genotype_util as gu
import pileup_util as pu
import quality_util as qu
import records_util as ru
import sweep_util as su
from bam_util import read_bam
from parity_util import assert_same_as_oracle

world = pytest.fixture(scope="module")(su.grid_world)


def _emu(world, preset, batch):
    return emu_util.map_batch(world.pidx, mapad_amd.make_params(qu.params(preset)), *batch)


@pytest.mark.parametrize("cid,preset", qu.CELLS, ids=qu.CELL_IDS)
def test_quality_and_alphabet_cases(world, cid, preset):
    batch = qu.case_batch(world, cid)
    ores = qu.oracle(world, cid, preset)
    print(cid, preset, qu.check_reach(cid, preset, ores, batch))
    if preset in qu.QUALITY_BLIND:
        qu.check_quality_blind(world, cid, preset)
    assert_same_as_oracle(ores, _emu(world, preset, batch), batch[2])


def test_quality_ladder_and_its_heaviest_read_through_the_host_tail(world):
    """Per-read quality centres from 0 to 255: the reads at Q0-Q5 take millions of pops (the slowest case of the file: the oracle's search and the emulation's).
    The heaviest of them once more through the host tail's search (csrc/host_tail.hpp: tail_search), which is what finishes such a read in production."""
    batch = qu.ladder_batch(world)
    ores = qu.ladder_oracle(world)
    counts, light = qu.check_ladder_reach(ores, batch)
    print("ladder", counts)
    res = _emu(world, "damage", batch)
    assert_same_as_oracle(ores, res, batch[2])
    heaviest = int(np.argmax(ores.counters[:, 3]))
    _, pops, status, _, _ = emu_util.tail_search(world.pidx, mapad_amd.make_params(qu.params("damage")), *batch, np.array([heaviest]), threads=1)
    assert int(pops[0]) == int(ores.counters[heaviest, 3]) >= su.GRID_MAX_POPS and int(status[0]) == int(res.status[heaviest])


@pytest.mark.parametrize("preset", ["damage", "no_damage", "continuous", "double_stranded"])
def test_model_rows_from_q92_up_are_one_row(preset):
    """e = seq_err + divergence - seq_err * divergence sits near the divergence constant (host_models.hpp: simple_adna_get), and towards Q90 its f32 ulp swallows
    seq_err: for the read lengths of the cases the rows of Q92 ... Q255 are bit-identical (the highest quality with a value of its own is 91, at position 17 of a
    35-base read under the damage presets; 86 without damage), so no search case can tell them apart and a clamp of the quality anywhere from 92 up changes nothing
    (DESIGN.md §2); what holds rows 94-255 of the tables is that `q255` and `full_byte` read them.  Q86 differs at every position.  Checked for every read length from
    35 to 70 at every position with Q92 / Q93 / Q94 / Q254 against Q255, and with every quality in between at the ends and the middle of 35-, 50- and 70-base reads.  A
    model change that makes rows 94-255 distinguishable fails here and asks for cases that distinguish them."""
    p = mapad_amd.make_params(qu.params(preset))
    get = mapad_amd.lib().mapad_sdm_get

    def row(L, pos, q):
        return np.array([np.float32(get(C.byref(p), pos, L, ord(f), ord(t), q)) for f in "ACGT" for t in "ACGT"]).view(np.uint32)

    for L in range(35, 71):
        for pos in range(L):
            top = row(L, pos, 255)
            for q in range(92, 255) if L in (35, 50, 70) and pos in (0, 1, L // 2, L - 1) else (92, 93, 94, 254):
                assert np.array_equal(row(L, pos, q), top), (L, pos, q)
            assert not np.array_equal(row(L, pos, 86), top), (L, pos)


@pytest.mark.parametrize("name", qu.ACC_BATCHES)
def test_host_accumulators_at_the_ends_of_the_quality_axis(world, name):
    """damage score, allele and genotype likelihoods and the pileup of the host path against their independent restatements (dscore_util, allele_util, genotype_util,
    pileup_util) on qualities over the whole byte, at 255 throughout and in {0, 1, 254, 255}"""
    batch = qu.acc_batch(world, name)
    p = mapad_amd.make_params(qu.params("damage"))
    lengths = [len(world.genome)]
    res = emu_util.map_batch(world.pidx, p, *batch)
    recs = mapad_amd.hits_to_records(world.pidx, p, res, *batch, seed=qu.ACC_SEED)
    counted = qu.m_column_qualities(recs, batch)
    qu.check_accumulator_reach(name, counted)
    score_q, scored, summary = mb.damage_score_host(world.pidx, p, res, *batch, seed=qu.ACC_SEED)
    want_q, want_scored, want = ds.from_records(p, recs, batch)
    assert np.array_equal(score_q, want_q) and np.array_equal(scored, want_scored) and (score_q != 0).any()
    ds.assert_summary(summary, want, name)
    acc = mb.AlleleHost(world.pidx, 1, genotypes=True).add(p, res, *batch, seed=qu.ACC_SEED)
    table = gu.from_records(p, lengths, recs, batch, 1)
    au.assert_equal(acc.summary(*qu.ACC_ALLELE_RULE), table, *qu.ACC_ALLELE_RULE, what=name, cells_of=acc.cells, consensus_of=acc.consensus)
    gu.assert_equal(acc, table, qu.ACC_GENOTYPE_RULE, name)
    by_min_bq = {}
    for min_bq in qu.ACC_MIN_BQ:
        pil = mb.PileupHost(world.pidx, 1, min_bq, 0, 0).add(p, res, *batch, seed=qu.ACC_SEED)
        by_min_bq[min_bq] = pil.summary(*qu.ACC_PILEUP_RULE)
        pu.assert_equal(by_min_bq[min_bq], pu.from_records(lengths, recs, batch, 1, min_bq), *qu.ACC_PILEUP_RULE, what=f"{name}, min_bq {min_bq}", counts_of=pil.counts, consensus_of=pil.consensus)
    qu.check_low_quality_moves(name, by_min_bq, counted)
    with pytest.raises(mapad_amd.MapadError):
        mb.PileupHost(world.pidx, 1, 256, 0, 0)


def test_command_line_inputs_through_the_host_path_and_recode(tmp_path):
    """The inputs of the GPU test's `mapad-amd map` runs — FASTQ quality strings over `!`..`~`, BAM records of 0xFF and of raw qualities 94-254 — without a GPU: the
    expectation's rows against the oracle's own text rows where those can hold the qualities, the host record path against the expectation (fixed fields and tags only:
    the host path lays out neither SEQ nor QUAL), and reader and writer (`mapad-amd recode`) byte for byte: the written QUAL is the input's."""
    rworld = qu.cli_world(str(tmp_path / "ref.fa"), subprocess.check_call)
    inputs = qu.cli_inputs(rworld.contigs[0][1])
    p = mapad_amd.make_params(qu.params(qu.CLI_PRESET))
    for form, recs in inputs.items():
        rows, ores = qu.cli_expectation(rworld, recs)
        qu.check_cli_reach(rows)
        if form == "fastq":
            for row, line in zip(rows, ores.records([r["flags"] for r in recs])):
                assert {k: str(v) for k, v in row.items()} == line
        batch = ob.pack_reads([r["seq"].encode() for r in recs], [qu.raw_quals(r) for r in recs])
        res = emu_util.map_batch(rworld.pidx, p, *batch)
        out = mapad_amd.hits_to_records(rworld.pidx, p, res, *batch, in_flags=np.array([r["flags"] for r in recs], np.uint16), seed=qu.CLI_SEED)
        n_bad, first, per_field = au_cli.compare([au_cli.host_record(r, inp) for r, inp in zip(out, recs)], rows, recs)
        assert n_bad == 0, au_cli.report(len(out), n_bad, first, per_field, form)
    for form, path in qu.cli_write_inputs(str(tmp_path), inputs).items():
        out = str(tmp_path / (form + ".out.bam"))
        subprocess.check_call([au_cli.cli(), "recode", "-r", path, "-o", out], stderr=subprocess.DEVNULL)
        got = read_bam(out)[2]
        n_bad, first, per_field = au_cli.compare(got, [None] * len(got), inputs[form])
        assert n_bad == 0, au_cli.report(len(got), n_bad, first, per_field, form)


@pytest.fixture(scope="module")
def record_world(world):
    return qu.record_world(world)


@pytest.mark.parametrize("preset", list(ru.PRESETS))
@pytest.mark.parametrize("cid", qu.RECORD_CASES)
def test_host_records_equal_the_oracles(world, record_world, cid, preset):
    """MAPQ takes its optimal scores from the base qualities (mapping.rs:570-590); MD and NM name the reference base under a read byte outside ACGT"""
    batch = qu.case_batch(world, cid)
    p = ru.params(preset)
    res = emu_util.map_batch(world.pidx, p, *batch)
    recs, text = mapad_amd.hits_to_records(world.pidx, p, res, *batch, seed=ru.SEED, as_arrays=True)
    n_bad, first, per_field = ru.differing((recs, text), record_world.oracle_canon(preset, res, batch))
    assert n_bad == 0, ru.report(first, per_field, f"{cid} {preset}")
    print(cid, preset, qu.check_record_reach(cid, world.genome, recs, text, batch))
