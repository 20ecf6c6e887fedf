"""The allele likelihoods without a GPU: the core driven directly (tests/emu/allele_selftest.cpp, a stand-alone program built with the address and
undefined-behaviour sanitizers), and mapad_allele_host_* (mapad_amd/csrc/allele_core.hpp — the source allele_kernel and allele_call_kernel compile too — over
the host's record_coords and the score tables built from the parameters) against cells, depths, skip counters, calls, qualities and per-contig statistics
built independently in numpy from the host records' contig, position, CIGAR, strand and XT, the reads, their qualities and mapad_allele_quantized_row
(tests/allele_util.py).  Reads are mapped by the host build of the kernels' per-read logic (tests/emu)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import synth

import allele_util as au
import emu_util
import pileup_util as pu
from kat_util import resolve_params
from parity_util import DAMAGE, IGNORE_BQ, VINDIJA

_HERE = os.path.dirname(os.path.abspath(__file__))
DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 717
SPLIT = 30_001
LENGTHS = [SPLIT, 60_000 - SPLIT]
TEST_MODEL = {"model": "test", "deam_score": -0.5, "mm_score": -1.0, "match_score": 0.0, "bound": "test", "threshold": -2.0, "repr_mm_bound": -1.0,
              "penalty_gap_open": -2.0, "penalty_gap_extend": -1.0, "gap_dist_ends": 5, "max_num_gaps_open": 1}
MODELS = {"ss": DAMAGE, "ignore_bq": IGNORE_BQ, "vindija": VINDIJA, "test_model": TEST_MODEL}
RULES = [(1, 3.0), (2, 0.0), (3, 10.5)]  # (min_depth, min_margin in bits)
FILTER = (25, 3, 2)


def make(model):
    return mapad_amd.make_params(resolve_params(model))


def test_core_selftest_under_sanitizers(tmp_path):
    """allele_quantize on ties, saturation and -0; the call rule on ties, a single allele, negative cells and margins near the int32 limits; a backward read's
    allele flip; a read ending on the last text position; a read one position past the text (flag raised, nothing written) — in a child process of its own"""
    exe = str(tmp_path / "allele_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(_HERE, "emu", "allele_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "allele selftest ok" in out.stdout, out.stdout + out.stderr


@pytest.fixture(scope="module")
def world():
    g = synth.genome(60_000, seed=41)
    g[25_000:25_300] = g[10_000:10_300]  # a repeat: reads from it have X0 > 1, so mode 2 drops reads that mode 1 counts
    return g, mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])


@pytest.fixture(scope="module")
def batch(world):
    g = world[0]
    ends = pu.hand_made([g[0:40], g[SPLIT - 40:SPLIT], g[SPLIT:SPLIT + 40], g[60_000 - 40:60_000], synth.revcomp(g[60_000 - 45:60_000]), synth.revcomp(g[SPLIT - 33:SPLIT])], qual=30)
    return pu.concat(synth.reads(g, 700, seed=7, qual_range=(2, 40), damage=DMG, len_range=(20, 140), indel_frac=0.3),
                     synth.reads(g[10_000:10_300], 80, 40, seed=8, exo_frac=0.0, damage=DMG), ends)


def mapped(world, batch, model):
    p = make(MODELS[model])
    res = emu_util.map_batch(world[1], p, *batch)
    return p, res, mapad_amd.hits_to_records(world[1], p, res, *batch, seed=SEED)


@pytest.fixture(scope="module")
def ss(world, batch):
    return mapped(world, batch, "ss")


def check_against_numpy(acc, want, what):
    for rule in RULES:
        au.assert_equal(acc.summary(*rule), want, *rule, what=f"{what}, rule {rule}", cells_of=acc.cells, consensus_of=acc.consensus)
    for t, (c, d) in enumerate(zip(want["ll"], want["depth"])):  # windows that start in the middle of a contig, on covered ground
        for start in (int(np.argmax(d)), LENGTHS[t] - 17):
            n = min(300, LENGTHS[t] - start)
            gl, gd = acc.cells(t, start, n)
            assert d[start] > 0 and np.array_equal(gl, c[start:start + n]) and np.array_equal(gd, d[start:start + n]), (what, t, start)
            gb, gq = acc.consensus(t, start, n, 2, 1.5)
            wb, wq = au.consensus(c[start:start + n], d[start:start + n], 2, 1.5)
            assert np.array_equal(gb, wb) and np.array_equal(gq, wq), (what, t, start)
    assert len(acc.cells(0, LENGTHS[0], 0)[1]) == 0 and len(acc.consensus(0, LENGTHS[0], 0)[0]) == 0


@pytest.mark.parametrize("model", list(MODELS))
def test_host_path_equals_the_table_built_from_the_records(world, batch, ss, model):
    g, idx = world
    p, res, recs = ss if model == "ss" else mapped(world, batch, model)
    rows = au.Rows(p)
    for mode, flt in ((1, (0, 0, 0)), (2, FILTER)):
        acc = mb.AlleleHost(idx, mode, *flt).add(p, res, *batch, seed=SEED)
        want = au.from_records(p, LENGTHS, recs, batch, mode, *flt, rows=rows)
        check_against_numpy(acc, want, f"{model}, mode {mode}, filters {flt}")
        s = acc.summary()
        n = len(batch[2]) - 1
        assert s["reads_seen"] == n and 0 < s["reads"] < n and s["batches"] == 1 and s["accumulate_ms"] == 0.0 and (s["mode"], s["min_base_quality"], s["mask5"], s["mask3"]) == (mode,) + flt
        assert s["min_depth"] == 1 and s["min_margin_q"] == 768 and s["columns_counted"] > 0
        assert all(0 < c["sites_called"] <= c["sites_covered"] < c["length"] and sum(c["called"]) == c["sites_called"] and c["margin_sum_q"] >= 768 * c["sites_called"]
                   for c in s["contigs"])
        if flt != (0, 0, 0):
            assert s["columns_masked"] > 0 and s["columns_low_quality"] > 0
    counted = [r for r in recs if r["mapped"]]
    assert {r["reverse"] for r in counted} == {False, True} and any(sum(int(k) for k, _ in pu._CIGAR.findall(r["cigar"])) > 64 for r in counted)
    if model != "test_model":
        assert any("D" in r["cigar"] for r in counted) and any("I" in r["cigar"] for r in counted)
    # the last bases of both contigs (the second one's is the text's last position) are covered, by both strands
    acc = mb.AlleleHost(idx, 1).add(p, res, *batch, seed=SEED)
    assert acc.cells(0, LENGTHS[0] - 1, 1)[1][0] >= 2 and acc.cells(1, LENGTHS[1] - 1, 1)[1][0] >= 2 and acc.cells(0, 0, 1)[1][0] >= 1


def test_quantized_rows_are_the_models_values(world):
    """one quality level: the quality byte does not matter; 256 levels: it does; every row is sdm_get rounded to 1/256 bit"""
    L = mapad_amd.lib()
    for model, nq in (("ss", 256), ("ignore_bq", 1)):
        p = make(MODELS[model])
        for (length, pos, q, to) in ((50, 0, 30, 3), (50, 25, 2, 1), (20, 19, 40, 0), (1, 0, 0, 2)):
            row = mapad_amd.allele_quantized_row(p, length, pos, q, to)
            want = [np.rint(np.float32(L.mapad_sdm_get(C.byref(p), pos, length, ord("ACGT"[f]), ord("ACGT"[to]), q if nq == 256 else 0)) * np.float32(256.0)) for f in range(4)]
            assert row.dtype == np.int16 and [int(x) for x in row] == [int(np.clip(w, -32768, 32767)) for w in want], (model, length, pos, q, to)
            other = mapad_amd.allele_quantized_row(p, length, pos, (q + 17) % 41, to)
            assert np.array_equal(other, row) == (nq == 1), (model, length, pos, q, to)
    p = make(DAMAGE)  # a 5' T over a reference C costs little, an interior T much; a Q2 base says next to nothing
    first, interior, q2 = (mapad_amd.allele_quantized_row(p, 50, pos, q, 3).astype(int) for pos, q in ((0, 30), (25, 30), (25, 2)))
    assert first[3] - first[1] < 3 * 256 <= interior[3] - interior[1] and abs(q2[3] - q2[1]) < 256


def test_depth_equals_the_sum_of_the_pileups_counts(world, batch, ss):
    g, idx = world
    p, res, _ = ss
    for mode, flt in ((1, (0, 0, 0)), (2, FILTER), (1, (0, 60, 60))):
        al = mb.AlleleHost(idx, mode, *flt).add(p, res, *batch, seed=SEED)
        pil = mb.PileupHost(idx, mode, *flt).add(p, res, *batch, seed=SEED)
        for t, n in enumerate(LENGTHS):
            assert np.array_equal(al.cells(t, 0, n)[1], pil.counts(t, 0, n).sum(axis=1, dtype=np.uint32)), (mode, flt, t)
        a, b = al.summary(), pil.summary()
        assert all(a[k] == b[k] for k in pu.SCALARS), (mode, flt)


def test_mode_2_skip_filters_and_batches(world, batch, ss):
    g, idx = world
    p, res, recs = ss
    n = len(batch[2]) - 1
    one, two = mb.AlleleHost(idx, 1).add(p, res, *batch, seed=SEED), mb.AlleleHost(idx, 2).add(p, res, *batch, seed=SEED)
    unique = sum(1 for r in recs if r["mapped"] and r["xt"] == "U")
    assert two.summary()["reads"] == unique < one.summary()["reads"] == sum(1 for r in recs if r["mapped"])
    # skip= leaves reads out: they are seen and nothing else
    skip = (np.arange(n) % 3 == 0).astype(np.uint8)
    acc = mb.AlleleHost(idx, 1).add(p, res, *batch, seed=SEED, skip=skip)
    want = au.from_records(p, LENGTHS, recs, batch, 1, skip=skip)
    au.assert_equal(acc.summary(), want, 1, 3.0, "skip", cells_of=acc.cells, consensus_of=acc.consensus)
    assert acc.summary()["reads_seen"] == n and acc.summary()["reads"] < one.summary()["reads"]
    with pytest.raises(ValueError):
        mb.AlleleHost(idx, 1).add(p, res, *batch, seed=SEED, skip=skip[:-1])
    # two batches add up to their concatenation
    import damage_util as du
    cut = n // 3
    a, b = du.take(batch, np.arange(cut)), du.take(batch, np.arange(cut, n))
    halves = mb.AlleleHost(idx, 1, *FILTER).add(p, emu_util.map_batch(idx, p, *a), *a, seed=SEED)
    halves.add(p, emu_util.map_batch(idx, p, *b), *b, seed=int(mapad_amd.lib().mapad_records_seed_at(SEED, cut)))
    whole = mb.AlleleHost(idx, 1, *FILTER).add(p, res, *batch, seed=SEED)
    au.assert_same_accumulators(halves, whole, LENGTHS, RULES, "two batches against one")
    assert halves.summary()["batches"] == 2
    # an accumulator holds the sums of one model
    with pytest.raises(mapad_amd.MapadError):
        whole.add(make(IGNORE_BQ), res, *batch, seed=SEED)


def test_the_boundary(world):
    L = mapad_amd.lib()
    names = ("mapad_ctx_set_allele_likelihoods", "mapad_ctx_allele_summary", "mapad_ctx_allele_cells", "mapad_ctx_allele_consensus", "mapad_ctx_allele_reset",
             "mapad_ctx_allele_merge", "mapad_allele_host_new", "mapad_allele_host_add", "mapad_allele_host_add_skip", "mapad_allele_host_summary", "mapad_allele_host_cells",
             "mapad_allele_host_consensus", "mapad_allele_host_free", "mapad_allele_quantized_row")
    for name in names:
        assert name in mb.SYMBOLS and hasattr(L, name)
    for name in ("set_allele_likelihoods", "allele_summary", "allele_cells", "allele_consensus", "allele_reset", "allele_merge"):
        assert hasattr(mapad_amd.Context, name)
    assert mapad_amd.AlleleHost is mb.AlleleHost and mapad_amd.allele_quantized_row is mb.allele_quantized_row
    out = mb.AlleleC()
    assert C.sizeof(mb.AlleleContigC) == 10 * 8 and C.sizeof(out) == 8 + 8 + 6 * 4 + 9 * 8 + 2 * 8
    buf = (C.c_uint32 * 16)()
    margin = C.c_float(3.0)
    assert L.mapad_ctx_set_allele_likelihoods(None, 1, 0, 0, 0) == -1 and L.mapad_ctx_allele_summary(None, 1, margin, C.byref(out)) == -1 and L.mapad_ctx_allele_reset(None) == -1
    assert L.mapad_ctx_allele_cells(None, 0, 0, 4, buf, buf) == -1 and L.mapad_ctx_allele_consensus(None, 0, 0, 4, 1, margin, buf, buf) == -1
    assert L.mapad_ctx_allele_merge(None, None) == -1
    h = C.c_void_p()
    assert L.mapad_allele_host_new(None, 1, 0, 0, 0, C.byref(h)) == -1 and L.mapad_allele_host_add(None, None, None, None, None, None, None, 0) == -1
    assert L.mapad_allele_host_summary(None, 1, margin, C.byref(out)) == -1 and L.mapad_allele_host_cells(None, 0, 0, 4, buf, buf) == -1
    assert L.mapad_allele_host_consensus(None, 0, 0, 4, 1, margin, buf, buf) == -1
    L.mapad_allele_host_free(None)
    p = make(DAMAGE)
    row = (C.c_int16 * 4)()
    for bad in ((0, 0, 30, 0), (32768, 0, 30, 0), (50, 50, 30, 0), (50, 0, 256, 0), (50, 0, 30, 4)):
        assert L.mapad_allele_quantized_row(C.byref(p), *bad, row) == -1, bad
    assert L.mapad_allele_quantized_row(None, 50, 0, 30, 0, row) == -1 and L.mapad_allele_quantized_row(C.byref(p), 50, 0, 30, 0, None) == -1
    _, idx = world
    for bad in ((0, 0, 0, 0), (3, 0, 0, 0), (1, 256, 0, 0), (1, 0, 65536, 0), (1, 0, 0, 65536)):  # mode 0 is not a host mode; filters beyond a quality / a read position
        with pytest.raises(mapad_amd.MapadError):
            mb.AlleleHost(idx, *bad)
    acc = mb.AlleleHost(idx, 1)
    nan = float("nan")
    for call in (lambda: acc.cells(0, LENGTHS[0] - 3, 4), lambda: acc.cells(2, 0, 1), lambda: acc.consensus(0, LENGTHS[0] - 3, 4), lambda: acc.consensus(0, 0, 4, 0, 3.0),
                 lambda: acc.consensus(0, 0, 4, 1, nan), lambda: acc.summary(0, 3.0), lambda: acc.summary(1, nan)):  # windows that leave their contig; min_depth 0; a margin that is no number
        with pytest.raises(mapad_amd.MapadError):
            call()
    zero = acc.summary(1, -4.0)  # a margin below one unit is one unit: nothing is called where nothing was counted
    assert zero["min_margin_q"] == 1 and zero["reads_seen"] == 0 and zero["batches"] == 0
    assert all(c["sites_covered"] == 0 and c["sites_called"] == 0 and c["max_depth"] == 0 and c["margin_sum_q"] == 0 for c in zero["contigs"])
    bases, quals = acc.consensus(1, 0, 5)
    assert bytes(bases) == b"NNNNN" and not quals.any()


def test_damaged_sites_are_called_wrong_less_often_than_by_the_majority_vote():
    """Meaning, in two directions and nothing else.  A synthetic genome, reads drawn from it with the single-stranded damage of the preset (f = t = 0.5,
    d = 0.02, s = 1.0) and without, at a mean depth of about 3; the truth is the genome.  Over the reference's C and G sites the share of wrong calls among the
    called sites is lower for the likelihood call (min_depth 1, the default margin of 3 bits) than for pileup_call (min_depth 1, min_percent 0, no masks); and on
    the undamaged draw the two callers agree wherever both call."""
    g = synth.genome(40_000, seed=53)
    idx = mapad_amd.Index.build([("chr", g)])
    p = make(DAMAGE)
    cg = (g == ord("C")) | (g == ord("G"))
    out = {}
    for name, damage in (("damaged", DMG), ("undamaged", None)):
        batch = synth.reads(g, 2400, 50, seed=61, subst_rate=0.001, exo_frac=0.0, qual_range=(20, 40), damage=damage)
        res = emu_util.map_batch(idx, p, *batch)
        al = mb.AlleleHost(idx, 1).add(p, res, *batch, seed=SEED)
        pil = mb.PileupHost(idx, 1).add(p, res, *batch, seed=SEED)
        a, v = al.consensus(0, 0, len(g))[0], pil.consensus(0, 0, len(g), 1, 0)
        out[name] = (a, v)
        ca, cv = (a != ord("N")) & cg, (v != ord("N")) & cg
        print("%s draw, reference C/G sites: likelihood call %d called, %d wrong; majority vote %d called, %d wrong; mean depth %.2f" %
              (name, int(ca.sum()), int((ca & (a != g)).sum()), int(cv.sum()), int((cv & (v != g)).sum()), al.summary()["columns_counted"] / len(g)))
        out[name + "_counts"] = (int(ca.sum()), int((ca & (a != g)).sum()), int(cv.sum()), int((cv & (v != g)).sum()))
    called_a, wrong_a, called_v, wrong_v = out["damaged_counts"]
    assert called_a > 1000 and called_v > 1000 and wrong_v > 0
    assert wrong_a * called_v < wrong_v * called_a  # wrong_a / called_a < wrong_v / called_v
    a, v = out["undamaged"]
    both = (a != ord("N")) & (v != ord("N"))
    assert both.sum() > 10_000 and np.array_equal(a[both], v[both]), np.flatnonzero(both & (a != v))[:10]
