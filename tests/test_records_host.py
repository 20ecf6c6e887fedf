"""The record-level parity cases of tests/records_util.py without a GPU: reads mapped by the host build of the kernels' per-read logic (tests/emu), records by the
host path (mapad_hits_to_records: host_postproc.hpp), compared field by field with the oracle's intervals_to_record over the same hits.  Proves the case table
that tests/test_gpu_records.py runs on the device, and keeps the host path honest on the same edges.  tests/emu/text_selftest.cpp drives the text kernel's
formatting code (text_core.hpp) directly."""
import os
import subprocess

import pytest

import mapad_amd

import emu_util
import records_util as ru
from parity_util import check_ungapped_records_against_the_text

_HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def a():
    world, clean = ru.world_a()
    batch, straddlers = ru.reads_a(world, clean)
    return world, clean, batch, straddlers


@pytest.mark.parametrize("preset", list(ru.PRESETS))
def test_world_a_host_records_equal_the_oracles(a, preset):
    world, clean, batch, straddlers = a
    p = ru.params(preset)
    res = emu_util.map_batch(world.pidx, p, *batch)
    recs, text = mapad_amd.hits_to_records(world.pidx, p, res, *batch, seed=ru.SEED, as_arrays=True)
    n_bad, first, per_field = ru.differing((recs, text), world.oracle_canon(preset, res, batch))
    counts = ru.edge_counts_a(world, recs, text, straddlers, res.hit_begin)
    print(preset, counts)
    assert n_bad == 0, ru.report(first, per_field)
    ru.check_reach_a(counts)
    checked, failed = check_ungapped_records_against_the_text(clean, ru.ungapped_text_check_input(world, recs, batch[2]), text, batch[0], batch[2], contig_starts=world.starts[:-1])
    assert checked > 1000 and failed == 0  # 1361 / 1363 ungapped records on code-free stretches


def test_world_b_caller_built_hit_lists_host_records_equal_the_oracles():
    world, text, starts = ru.world_b()
    batch = ru.reads_b(text, starts)
    p = ru.params(ru.B_PRESET)
    cres = ru.hit_lists_b(emu_util.map_batch(world.pidx, p, *batch))
    recs, rtext = mapad_amd.hits_to_records(world.pidx, p, cres, *batch, seed=ru.SEED, as_arrays=True)
    n_bad, first, per_field = ru.differing((recs, rtext), world.oracle_canon(ru.B_PRESET, cres, batch))
    counts = ru.edge_counts_b(cres, recs)
    print(counts, "pairs", ru.pairs_needed(cres, recs), "initial pools", ru.initial_pools(cres.n_reads))
    assert n_bad == 0, ru.report(first, per_field)
    ru.check_reach_b(counts)
    # what the GPU test of the pool-overflow rerun needs of this world
    text_cap, pair_cap = ru.initial_pools(cres.n_reads)
    assert counts["text_bytes"] > 2 * text_cap and ru.pairs_needed(cres, recs) > 2 * pair_cap
    for edited in ru.edge_batches_b(cres).values():  # the wavefront-edge batches of the GPU test are sound on the reference side too
        got = mapad_amd.hits_to_records(world.pidx, p, edited, *batch, seed=ru.SEED, as_arrays=True)
        n_bad, first, per_field = ru.differing(got, world.oracle_canon(ru.B_PRESET, edited, batch))
        assert n_bad == 0, ru.report(first, per_field)


def test_text_selftest_under_sanitizers(tmp_path):
    """TextSink::put_f2 / put_u64 against snprintf, bam_fields_hd against host::to_bam_fields on hand-written tracks (an insertion in front of an original symbol, a
    deletion run across one, 19 consecutive symbols, every code on the reverse strand, 32 767 operations) — in a child process of its own"""
    exe = str(tmp_path / "text_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-pthread", "-o", exe, os.path.join(_HERE, "emu", "text_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "text selftest ok" in out.stdout, out.stdout + out.stderr
