"""The damage score without a GPU: the table (mapad_damage_score_table) against the models' formulas in numpy float64, the core driven directly
(tests/emu/dscore_selftest.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers), and mapad_damage_score_host
(mapad_amd/csrc/dscore_core.hpp — the source dscore_kernel compiles too — over the host's record_coords) against scores decoded independently from the host
records' CIGAR / MD / strand, the reads and their qualities (tests/dscore_util.py).  Reads are mapped by the host build of the kernels' per-read logic (tests/emu)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import synth

import dscore_util as ds
import emu_util
from kat_util import resolve_params
from parity_util import DAMAGE, DOUBLE_STRANDED, IGNORE_BQ, NO_DAMAGE, VINDIJA

_HERE = os.path.dirname(os.path.abspath(__file__))
DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 4242
TEST_MODEL = {"model": "test", "deam_score": -0.5, "mm_score": -1.0, "match_score": 0.0, "bound": "test", "threshold": -2.0, "repr_mm_bound": -1.0,
              "penalty_gap_open": -2.0, "penalty_gap_extend": -1.0, "gap_dist_ends": 5, "max_num_gaps_open": 1}
MODELS = {"ss": DAMAGE, "ds": DOUBLE_STRANDED, "test_model": TEST_MODEL}
LENGTHS = (1, 20, 50, 70)


def make(model):
    return mapad_amd.make_params(resolve_params(model))


def test_core_selftest_under_sanitizers(tmp_path):
    """the column rule on hand-made tracks (p >= L, N, lower case, insertions and deletions, L = 1), int16 saturation under an extreme test-model score, the
    rounding of the table and of the threshold, the bin rule at -9000, -8192, -1, 0, 127, 128, 8191, 9000 — in a child process of its own"""
    exe = str(tmp_path / "dscore_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(_HERE, "emu", "dscore_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "dscore selftest ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("model", list(MODELS) + ["ignore_bq", "vindija"])
def test_table_equals_the_formula_in_float64(model):
    """Every cell within one unit of 1/256 bit: the f32 error of a log2 difference is ~1e-5 bits, far below a unit, so only a value that lands on a rounding
    tie can come out one unit apart."""
    p = make({"ignore_bq": IGNORE_BQ, "vindija": VINDIJA}.get(model) or MODELS[model])
    for L in LENGTHS:
        got = mapad_amd.damage_score_table(p, L)
        want = ds.table_f64(p, L)
        assert got.dtype == np.int16 and got.shape == want.shape == (L, 256 if model in ("ss", "ds") else 1, 4)
        diff = np.abs(got.astype(np.float64) - np.rint(want))
        print(model, L, "largest difference in units:", diff.max(), "cells one unit apart:", int((diff == 1).sum()), "of", diff.size)
        assert diff.max() <= 1, (model, L, np.argwhere(diff > 1)[:5])
    if model == "test_model":  # C->T scores -0.5 instead of -1.0: half a bit, everything else nothing
        assert np.array_equal(mapad_amd.damage_score_table(p, 20), np.tile(np.array([0, 128, 0, 0], np.int16), (20, 1, 1)))
    if model == "ss":  # G->A at the double-stranded rate wherever it is: no position in it; damage makes C->T likelier and C->C less likely at both ends
        t = mapad_amd.damage_score_table(p, 50)
        assert (t[:, :, 2:] == t[:1, :, 2:]).all() and (t[0, 20:, 1] > 0).all() and (t[0, 20:, 0] < 0).all() and (t[49, 20:, 1] > 0).all()


def test_table_without_damage_is_zero():
    for base in (NO_DAMAGE, dict(DOUBLE_STRANDED, ds_deamination_rate=0.0, ss_deamination_rate=0.0), dict(IGNORE_BQ, ds_deamination_rate=0.0, ss_deamination_rate=0.0)):
        p = make(base)
        for L in LENGTHS:
            assert not mapad_amd.damage_score_table(p, L).any()


def test_double_stranded_cells_depend_on_the_distance_from_their_end_only():
    """C cells on the distance from the 5' end, G cells on the distance from the 3' end: equal across read lengths"""
    p = make(DOUBLE_STRANDED)
    tabs = {L: mapad_amd.damage_score_table(p, L) for L in LENGTHS}
    assert tabs[70][:, :, 1].any() and tabs[70][:, :, 3].any()
    for a in LENGTHS:
        for b in LENGTHS:
            if a < b:
                assert np.array_equal(tabs[a][:, :, :2], tabs[b][:a, :, :2])
                assert np.array_equal(tabs[a][::-1, :, 2:], tabs[b][::-1, :, 2:][:a])


@pytest.fixture(scope="module")
def world():
    g = synth.genome(400_000, seed=77)
    g[300_000:300_400] = g[100_000:100_400]
    return g, mapad_amd.Index.build([("c1", g[:250_000]), ("c2", g[250_000:])])


@pytest.fixture(scope="module")
def batch(world):
    return synth.reads(world[0], 6000, seed=5, qual_range=(20, 40), damage=DMG, len_range=(20, 70), indel_frac=0.2)


@pytest.fixture(scope="module")
def ss_scores(world, batch):
    g, idx = world
    p = make(DAMAGE)
    res = emu_util.map_batch(idx, p, *batch)
    return p, res, mb.damage_score_host(idx, p, res, *batch, seed=SEED)


@pytest.mark.parametrize("model", list(MODELS))
def test_host_scores_equal_the_scores_decoded_from_the_records(world, batch, ss_scores, model):
    g, idx = world
    if model == "ss":
        p, res, (score_q, scored, summary) = ss_scores
    else:
        p = make(MODELS[model])
        res = emu_util.map_batch(idx, p, *batch)
        score_q, scored, summary = mb.damage_score_host(idx, p, res, *batch, seed=SEED)
    recs = mapad_amd.hits_to_records(idx, p, res, *batch, seed=SEED)
    want_q, want_scored, want = ds.from_records(p, recs, batch)
    assert np.array_equal(scored, want_scored) and np.array_equal(score_q, want_q), np.flatnonzero(score_q != want_q)[:10]
    ds.assert_summary(summary, want, model)
    n = len(batch[2]) - 1
    assert summary["batches"] == 1 and summary["reads_seen"] == n and 0 < summary["reads_scored"] < n and summary["kernel_ms"] == 0.0 and summary["threshold_q"] == 0
    assert int(summary["histogram"].sum()) == summary["reads_scored"] and summary["informative_columns"] > summary["reads_scored"]
    assert not score_q[scored == 0].any()
    mapped = [r for r in recs if r["mapped"]]
    assert any(r["reverse"] for r in mapped) and any(not r["reverse"] for r in mapped)  # both strands
    if model != "test_model":
        assert any("I" in r["cigar"] for r in mapped) and any("D" in r["cigar"] for r in mapped)
    assert (score_q > 0).any() and ((score_q < 0).any() or model == "test_model")
    assert "damage_score" not in recs[0]  # the host records path carries no scores


def test_damaged_reads_score_higher_than_undamaged_ones(world, batch, ss_scores):
    """The meaning of the sign, with no absolute value asserted: on the same genome under the same parameters the mean score of reads drawn with damage is
    strictly higher than that of reads drawn without."""
    g, idx = world
    p, _, (score_q, scored, _) = ss_scores
    plain = synth.reads(g, 2000, seed=6, qual_range=(20, 40), damage=None, len_range=(20, 70), indel_frac=0.2)
    res = emu_util.map_batch(idx, p, *plain)
    pq, ps, _ = mb.damage_score_host(idx, p, res, *plain, seed=SEED)
    with_damage, without = score_q[scored == 1].mean() / 256.0, pq[ps == 1].mean() / 256.0
    print("mean damage score in bits: reads with damage %.4f (%d scored), reads without %.4f (%d scored)" % (with_damage, int(scored.sum()), without, int(ps.sum())))
    assert scored.sum() > 1000 and ps.sum() > 300
    assert with_damage > without


def test_threshold_and_two_batches(world, batch, ss_scores):
    g, idx = world
    p, res, (score_q, scored, summary) = ss_scores
    # ceilf at exact and inexact values
    for thr, want in ((3.0, 768), (0.0, 0), (0.1, 26), (-0.1, -25), (1.0 / 256.0, 1), (float(np.nextafter(np.float32(1.0 / 256.0), np.float32(1.0))), 2), (-3.0, -768)):
        q, s, d = mb.damage_score_host(idx, p, res, *batch, seed=SEED, threshold=thr)
        assert d["threshold_q"] == want and d["reads_below"] == int(((score_q < want) & (scored == 1)).sum()), thr
        assert np.array_equal(q, score_q) and np.array_equal(s, scored)  # the threshold changes no score
    assert 0 < mb.damage_score_host(idx, p, res, *batch, seed=SEED, threshold=float(np.median(score_q[scored == 1])) / 256.0)[2]["reads_below"] < summary["reads_scored"]
    # two batches add up to their concatenation
    n = len(batch[2]) - 1
    cut = n // 3
    import damage_util as du
    a, b = du.take(batch, np.arange(cut)), du.take(batch, np.arange(cut, n))
    qa, sa, d = mb.damage_score_host(idx, p, emu_util.map_batch(idx, p, *a), *a, seed=SEED, threshold=1.0)
    qb, sb, d = mb.damage_score_host(idx, p, emu_util.map_batch(idx, p, *b), *b, seed=int(mapad_amd.lib().mapad_records_seed_at(SEED, cut)), threshold=1.0, into=d)
    one = mb.damage_score_host(idx, p, res, *batch, seed=SEED, threshold=1.0)[2]
    assert np.array_equal(np.concatenate([qa, qb]), score_q) and np.array_equal(np.concatenate([sa, sb]), scored)
    ds.assert_summary(d, dict(one, batches=2), "two batches against one")


def test_the_boundary(world, batch, ss_scores):
    g, idx = world
    p, res, _ = ss_scores
    L = mapad_amd.lib()
    names = ("mapad_ctx_set_damage_score", "mapad_ctx_damage_scores", "mapad_ctx_damage_scores_reset", "mapad_records_damage_scores", "mapad_damage_score_host",
             "mapad_damage_score_table")
    for name in names:
        assert name in mb.SYMBOLS and hasattr(L, name)
    for name in ("set_damage_score", "damage_scores", "reset_damage_scores"):
        assert hasattr(mapad_amd.Context, name)
    assert mapad_amd.damage_score_host is mb.damage_score_host and mapad_amd.damage_score_table is mb.damage_score_table
    out = mb.DamageScoresC()
    assert C.sizeof(out) == 6 * 8 + 2 * 4 + 128 * 8 + 8
    assert L.mapad_ctx_set_damage_score(None, 1, 0.0) == -1 and L.mapad_ctx_damage_scores(None, C.byref(out)) == -1 and L.mapad_ctx_damage_scores_reset(None) == -1
    nq = C.c_int()
    assert L.mapad_damage_score_table(None, 50, None, C.byref(nq)) == -1 and L.mapad_damage_score_table(C.byref(p), 0, None, C.byref(nq)) == -1
    assert L.mapad_damage_score_table(C.byref(p), 32768, None, C.byref(nq)) == -1 and L.mapad_damage_score_table(C.byref(p), 50, None, None) == -1
    assert L.mapad_damage_score_table(C.byref(p), 50, None, C.byref(nq)) == 0 and nq.value == 256
    assert L.mapad_damage_score_host(None, None, None, None, None, None, 0, 0.0, None, None, None) == -1
    assert L.mapad_damage_score_host(idx.h, C.byref(p), res._cptr, None, None, None, 0, 0.0, None, None, None) == -1  # reads, and nothing to score them from
    with pytest.raises(mapad_amd.MapadError):
        mb.damage_score_host(idx, p, res, *batch, seed=SEED, threshold=float("nan"))
    # the host records carry no scores: NULL pointers
    recs = C.POINTER(mb.RecordsC)()
    seqs, quals, offsets = (np.ascontiguousarray(x) for x in batch)
    assert L.mapad_hits_to_records(idx.h, C.byref(p), res._cptr, seqs.ctypes.data, quals.ctypes.data, offsets.ctypes.data, None, SEED, C.byref(recs)) == 0
    sq, sc = C.c_void_p(1), C.c_void_p(1)
    assert L.mapad_records_damage_scores(recs, C.byref(sq), C.byref(sc)) == 0 and sq.value is None and sc.value is None
    assert L.mapad_records_damage_scores(None, C.byref(sq), C.byref(sc)) == -1 and L.mapad_records_damage_scores(recs, None, None) == -1
    L.mapad_records_free(recs)
