"""Quality rescaling without a GPU: the table (mapad_quality_rescale_table) against the rule restated in numpy float64, the core driven directly
(tests/emu/rescale_selftest.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers), and mapad_quality_rescale_host
(mapad_amd/csrc/rescale_core.hpp — the source rescale_kernel compiles too — over the host's record_coords) against qualities decoded independently from the host
records' CIGAR / MD / strand, the reads and their qualities (tests/rescale_util.py).  Reads are mapped by the host build of the kernels' per-read logic (tests/emu)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import synth

import damage_util as du
import emu_util
import rescale_util as ru
from kat_util import resolve_params
from parity_util import DAMAGE, DOUBLE_STRANDED, IGNORE_BQ, NO_DAMAGE, VINDIJA

_HERE = os.path.dirname(os.path.abspath(__file__))
DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 4242
TEST_MODEL = {"model": "test", "deam_score": -0.5, "mm_score": -1.0, "match_score": 0.0, "bound": "test", "threshold": -2.0, "repr_mm_bound": -1.0,
              "penalty_gap_open": -2.0, "penalty_gap_extend": -1.0, "gap_dist_ends": 5, "max_num_gaps_open": 1}
MODELS = {"ss": DAMAGE, "ds": DOUBLE_STRANDED, "ignore_bq": IGNORE_BQ, "vindija": VINDIJA, "test_model": TEST_MODEL}
LENGTHS = (1, 20, 50, 70)
NEAR_HALF = 1e-6  # an entry whose float64 value lies this close to a half-integer may come out one apart
MAX_NEAR = 8      # ... and a table may have at most this many of them


def make(model):
    return mapad_amd.make_params(resolve_params(model))


def test_core_selftest_under_sanitizers(tmp_path):
    """the column rule on hand-made tracks (p >= L, N and lower case, a mismatch behind an insertion and behind a deletion, L = 1), quality bytes 0, 1, 93, 94, 254
    and 255, e' >= 1, the identity without damage — in a child process of its own"""
    exe = str(tmp_path / "rescale_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(_HERE, "emu", "rescale_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "rescale selftest ok" in out.stdout, out.stdout + out.stderr


def _near_half(raw):
    """entries whose value before the floor, -10 log10(e') + 0.5, lies within NEAR_HALF of an integer: -10 log10(e') within NEAR_HALF of a half-integer"""
    fin = np.isfinite(raw)
    return fin & (np.abs(raw - np.rint(np.where(fin, raw, 0.0))) < NEAR_HALF)


@pytest.mark.parametrize("model", list(MODELS))
def test_table_equals_the_rule_in_float64(model):
    p = make(MODELS[model])
    for L in LENGTHS:
        got = mapad_amd.quality_rescale_table(p, L)
        raw, want = ru.table_f64(p, L)
        assert got.dtype == np.uint8 and got.shape == want.shape == (L, 256, 2)
        near = _near_half(raw)
        diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
        print(model, L, "entries near a half-integer:", int(near.sum()), "entries that differ:", int((diff != 0).sum()), "of", diff.size, "changed by the rule:",
              int((want != np.arange(256, dtype=np.uint8)[None, :, None]).sum()))
        assert near.sum() <= MAX_NEAR, (model, L, np.argwhere(near)[:10])
        assert not diff[~near].any(), (model, L, np.argwhere((diff != 0) & ~near)[:5])
        assert diff.max() <= 1
        assert (got[:, 255, :] == 255).all()
    t = mapad_amd.quality_rescale_table(p, 50)
    ident = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], t.shape)
    assert (t[:, :255, 0] < ident[:, :255, 0]).any()  # C->T is marked down under every one of these models
    if model in ("vindija", "test_model"):  # no G->A damage in them
        assert np.array_equal(t[:, :, 1], ident[:, :, 1])
    if model in ("ss", "ignore_bq"):  # G->A sees the -d rate at every position: no position in it, and it does change something
        assert (t[:, :, 1] == t[:1, :, 1]).all() and (t[0, :255, 1] < ident[0, :255, 1]).any()
        assert t[0, 37, 0] < t[25, 37, 0] and t[49, 37, 0] < t[25, 37, 0]  # both ends of a single-stranded read are marked down further than its middle
    if model == "ds":  # C->T by the distance from the 5' end, G->A by the distance from the 3' end
        assert np.array_equal(t[:, :, 0], t[::-1, :, 1]) and t[0, 37, 0] < t[49, 37, 0]


def test_the_formula_has_no_entry_near_a_half_integer_at_the_usual_settings():
    """f = t = 0.5, d = 0.02, s = 1.0, divergence = 0.02 / 3, Q0..93, L of 20, 50 and 129, both library types: nothing within 1e-6 of a half-integer"""
    for base in (DAMAGE, DOUBLE_STRANDED):
        p = make(base)  # (these are the settings of both presets)
        assert (p.five_prime_overhang, p.three_prime_overhang, p.ss_deamination_rate) == (0.5, 0.5, 1.0) and p.ds_deamination_rate == np.float32(0.02)
        for L in (20, 50, 129):
            raw, want = ru.table_f64(p, L)
            assert not _near_half(raw[:, :94, :]).any()
            assert np.array_equal(mapad_amd.quality_rescale_table(p, L)[:, :94, :], want[:, :94, :])


def test_table_without_damage_is_the_identity():
    ident = np.arange(256, dtype=np.uint8)[None, :, None]
    for base in (NO_DAMAGE, dict(DOUBLE_STRANDED, ds_deamination_rate=0.0, ss_deamination_rate=0.0), dict(IGNORE_BQ, ds_deamination_rate=0.0, ss_deamination_rate=0.0),
                 dict(TEST_MODEL, deam_score=-1.0), dict(TEST_MODEL, deam_score=-3.0)):  # (the test model: C->T scored like, or below, any mismatch)
        p = make(base)
        for L in LENGTHS:
            t = mapad_amd.quality_rescale_table(p, L)
            assert np.array_equal(t, np.broadcast_to(ident, t.shape)), (base, L)


@pytest.mark.parametrize("model", list(MODELS))
def test_never_raises_a_quality(model):
    p = make(MODELS[model])
    for L in LENGTHS + (129,):
        t = mapad_amd.quality_rescale_table(p, L)
        assert (t <= np.arange(256, dtype=np.uint8)[None, :, None]).all()


@pytest.fixture(scope="module")
def world():
    g = synth.genome(400_000, seed=77)
    g[300_000:300_400] = g[100_000:100_400]
    return g, mapad_amd.Index.build([("c1", g[:250_000]), ("c2", g[250_000:])])


@pytest.fixture(scope="module")
def batch(world):
    seqs, quals, offsets = synth.reads(world[0], 4000, seed=5, qual_range=(20, 40), damage=DMG, len_range=(20, 70), indel_frac=0.2)
    quals = quals.copy()
    quals[::97] = 255  # missing qualities, 0 and 93 among the usual ones
    quals[1::101] = 0
    quals[2::103] = 93
    return seqs, quals, offsets


@pytest.mark.parametrize("model", ["ss", "ds", "test_model"])
def test_host_path_equals_the_qualities_decoded_from_the_records(world, batch, model):
    g, idx = world
    p = make(MODELS[model])
    res = emu_util.map_batch(idx, p, *batch)
    out, summary = mb.quality_rescale_host(idx, p, res, *batch, seed=SEED)
    recs = mapad_amd.hits_to_records(idx, p, res, *batch, seed=SEED)
    want_out, want = ru.from_records(p, recs, batch)
    assert out.dtype == np.uint8 and np.array_equal(out, want_out), np.flatnonzero(out != want_out)[:10]
    ru.assert_summary(summary, want, model)
    seqs, quals, offsets = batch
    n = len(offsets) - 1
    assert summary["batches"] == 1 and summary["reads_seen"] == n and 0 < summary["reads_rescaled"] < n and summary["kernel_ms"] == 0.0
    changed = out != quals
    assert summary["bases_changed"] == int(changed.sum()) and 0 < changed.sum() < summary["candidate_columns"].sum() + 1
    assert (out <= quals).all() and summary["quality_drop_sum"] == int((quals.astype(np.int64) - out).sum()) and int(summary["new_quality"].sum()) == summary["bases_changed"]
    assert (out[quals == 255] == 255).all()
    mapped = np.array([r["mapped"] for r in recs])
    for r in np.flatnonzero(~mapped):  # every other read keeps its qualities
        assert not changed[int(offsets[r]):int(offsets[r + 1])].any()
    m = [r for r in recs if r["mapped"]]
    assert any(r["reverse"] for r in m) and any(not r["reverse"] for r in m)  # both strands
    if model != "test_model":
        assert any("I" in r["cigar"] for r in m) and any("D" in r["cigar"] for r in m)
        assert summary["candidate_columns"][0] > 0 and summary["candidate_columns"][1] > 0
    # no output array: the same summary
    acc = mb.RescaleC()
    seqs_c, quals_c, offsets_c = (np.ascontiguousarray(x) for x in batch)
    assert mapad_amd.lib().mapad_quality_rescale_host(idx.h, C.byref(p), res._cptr, seqs_c.ctypes.data, quals_c.ctypes.data, offsets_c.ctypes.data, SEED, None, C.byref(acc)) == 0
    ru.assert_summary(mb._rescale_dict(acc), summary, "without an output array")


def test_two_batches_add_into_one_accumulator(world, batch):
    g, idx = world
    p = make(DAMAGE)
    res = emu_util.map_batch(idx, p, *batch)
    out, one = mb.quality_rescale_host(idx, p, res, *batch, seed=SEED)
    n = len(batch[2]) - 1
    cut = n // 3
    a, b = du.take(batch, np.arange(cut)), du.take(batch, np.arange(cut, n))
    qa, d = mb.quality_rescale_host(idx, p, emu_util.map_batch(idx, p, *a), *a, seed=SEED)
    qb, d = mb.quality_rescale_host(idx, p, emu_util.map_batch(idx, p, *b), *b, seed=int(mapad_amd.lib().mapad_records_seed_at(SEED, cut)), into=d)
    assert np.array_equal(np.concatenate([qa, qb]), out)
    ru.assert_summary(d, dict(one, batches=2), "two batches against one")


def test_the_boundary(world, batch):
    g, idx = world
    p = make(DAMAGE)
    res = emu_util.map_batch(idx, p, *du.take(batch, np.arange(200)))
    small = du.take(batch, np.arange(200))
    L = mapad_amd.lib()
    names = ("mapad_ctx_set_quality_rescale", "mapad_ctx_quality_rescale", "mapad_ctx_quality_rescale_reset", "mapad_records_rescaled_quals", "mapad_quality_rescale_host",
             "mapad_quality_rescale_table")
    for name in names:
        assert name in mb.SYMBOLS and hasattr(L, name)
    for name in ("set_quality_rescale", "quality_rescale", "reset_quality_rescale"):
        assert hasattr(mapad_amd.Context, name)
    assert mapad_amd.quality_rescale_host is mb.quality_rescale_host and mapad_amd.quality_rescale_table is mb.quality_rescale_table
    out = mb.RescaleC()
    assert C.sizeof(out) == (2 + 2 + 2 + 64 + 1) * 8 + 8
    assert L.mapad_ctx_set_quality_rescale(None, 1) == -1 and L.mapad_ctx_quality_rescale(None, C.byref(out)) == -1 and L.mapad_ctx_quality_rescale_reset(None) == -1
    buf = np.zeros((50, 256, 2), np.uint8)
    assert L.mapad_quality_rescale_table(None, 50, buf.ctypes.data) == -1 and L.mapad_quality_rescale_table(C.byref(p), 0, buf.ctypes.data) == -1
    assert L.mapad_quality_rescale_table(C.byref(p), 32768, buf.ctypes.data) == -1 and L.mapad_quality_rescale_table(C.byref(p), 50, None) == -1
    assert L.mapad_quality_rescale_table(C.byref(p), 50, buf.ctypes.data) == 0 and np.array_equal(buf, mapad_amd.quality_rescale_table(p, 50))
    assert L.mapad_quality_rescale_host(None, None, None, None, None, None, 0, None, None) == -1
    assert L.mapad_quality_rescale_host(idx.h, C.byref(p), res._cptr, None, None, None, 0, None, None) == -1  # reads, and nothing to rescale
    # the host records carry no rescaled qualities: a NULL pointer
    recs = C.POINTER(mb.RecordsC)()
    seqs, quals, offsets = (np.ascontiguousarray(x) for x in small)
    assert L.mapad_hits_to_records(idx.h, C.byref(p), res._cptr, seqs.ctypes.data, quals.ctypes.data, offsets.ctypes.data, None, SEED, C.byref(recs)) == 0
    q, n = C.c_void_p(1), C.c_uint64(1)
    assert L.mapad_records_rescaled_quals(recs, C.byref(q), C.byref(n)) == 0 and q.value is None and n.value == 0
    assert L.mapad_records_rescaled_quals(None, C.byref(q), C.byref(n)) == -1 and L.mapad_records_rescaled_quals(recs, None, None) == -1
    L.mapad_records_free(recs)
