"""Depth of coverage without a GPU: mapad_coverage_host_* (mapad_amd/csrc/coverage_core.hpp — the source coverage_kernel compiles too — over the host's
record_coords, and the finishing pass restated serially over the same segments) against per-base depth built independently in numpy from the host records'
contig, position, CIGAR and XT (tests/coverage_util.py).  Reads are mapped by the host build of the kernels' per-read logic (tests/emu)."""
import ctypes as C

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import synth

import coverage_util as cu
import emu_util
from kat_util import resolve_params
from parity_util import DAMAGE

DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 777
SPLIT = 70_001  # where the two contigs meet: no multiple of a segment size used here (64, 1000, 16384)
LENGTHS = [SPLIT, 150_000 - SPLIT]


@pytest.fixture(scope="module")
def world():
    g = synth.genome(150_000, seed=31)
    g[60_000:60_300] = g[20_000:20_300]  # a repeat: reads from it have X0 > 1, so mode 2 drops reads that mode 1 counts
    idx = mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    return g, idx, params


def hand_made(g):
    """a read on base 0 of each contig, one ending on each contig's last base, one across a segment boundary of each size (1000 = 1000, 1024 = 16 x 64; 16384)"""
    return cu.hand_made([g[0:40], g[SPLIT:SPLIT + 40], g[SPLIT - 40:SPLIT], g[150_000 - 40:150_000], synth.revcomp(g[SPLIT - 45:SPLIT]), g[980:1040], g[16_360:16_410],
                         g[SPLIT + 990:SPLIT + 1030]])


@pytest.fixture(scope="module")
def mapped(world):
    g, idx, params = world
    batch = cu.concat(synth.reads(g, 1300, seed=7, qual_range=(20, 40), damage=DMG, len_range=(20, 150), indel_frac=0.3),
                      synth.reads(g[20_000:20_300], 150, 40, seed=8, exo_frac=0.0, damage=DMG), hand_made(g))
    res = emu_util.map_batch(idx, params, *batch)
    recs = mapad_amd.hits_to_records(idx, params, res, *batch, seed=SEED)
    return batch, res, recs


def host(world, res, mode, seed=SEED, into=None):
    _, idx, params = world
    acc = into if into is not None else mb.CoverageHost(idx, mode)
    return acc.add(params, res, seed=seed)


@pytest.mark.parametrize("mode", [1, 2])
def test_host_summary_and_depth_equal_the_table_built_from_the_records(world, mapped, mode):
    batch, res, recs = mapped
    acc = host(world, res, mode)
    got, want = acc.summary(), cu.from_records(LENGTHS, recs, mode)
    cu.assert_equal(got, want, f"mode {mode}", depth_of=acc.depth)
    n = len(batch[2]) - 1
    assert got["reads_seen"] == n and 0 < got["reads"] < n and got["batches"] == 1
    assert got["deleted_columns"] > 0 and got["insertions"] > 0
    assert sum(c["depth_sum"] for c in got["contigs"]) == got["covered_columns"]
    assert int(got["hist"].sum()) == sum(LENGTHS) and [c["length"] for c in got["contigs"]] == LENGTHS
    assert [c["name"] for c in got["contigs"]] == ["c1", "c2"] and all(c["reads"] > 0 for c in got["contigs"])
    # the world is what it is meant to be: tracks longer than one pass of a wavefront, deletions on both strands, the contigs' first and last bases covered
    counted = [r for r in recs if r["mapped"] and (mode == 1 or r["xt"] == "U")]
    assert any(sum(int(n) for n, _ in cu._CIGAR.findall(r["cigar"])) > 64 for r in counted)
    assert {r["reverse"] for r in counted if "D" in r["cigar"]} == {False, True}
    for t, d in enumerate(want["depth"]):
        assert d[0] > 0 and d[-1] > 0, t
    # windows that start in the middle of a contig, at non-zero depth
    for t, d in enumerate(want["depth"]):
        for start in (int(np.argmax(d)), int(np.flatnonzero(d)[len(np.flatnonzero(d)) // 2]), LENGTHS[t] - 17):
            n_win = min(700, LENGTHS[t] - start)
            assert d[start] > 0 and np.array_equal(acc.depth(t, start, n_win).astype(np.int64), d[start:start + n_win]), (t, start)
    assert len(acc.depth(0, LENGTHS[0], 0)) == 0


def test_unique_mode_counts_fewer_reads_and_is_nowhere_deeper(world, mapped):
    _, res, _ = mapped
    all_reads, unique = host(world, res, 1), host(world, res, 2)
    a, u = all_reads.summary(), unique.summary()
    assert u["reads"] < a["reads"] and u["reads_seen"] == a["reads_seen"]
    for t, n in enumerate(LENGTHS):
        assert (unique.depth(t, 0, n) <= all_reads.depth(t, 0, n)).all()


def test_two_batches_add_up_to_their_concatenation(world):
    g, idx, params = world
    a = synth.reads(g, 500, seed=10, qual_range=(20, 40), damage=DMG, len_range=(25, 90), indel_frac=0.3)
    b = cu.concat(synth.reads(g, 300, seed=11, qual_range=(20, 40), damage=DMG, len_range=(25, 60), indel_frac=0.2), synth.reads(g[20_000:20_300], 60, 40, seed=12, exo_frac=0.0))
    ab = cu.concat(a, b)
    res_a, res_b, res_ab = (emu_util.map_batch(idx, params, *x) for x in (a, b, ab))
    seed_b = int(mapad_amd.lib().mapad_records_seed_at(SEED, len(a[2]) - 1))
    for mode in (1, 2):
        one = host(world, res_ab, mode)
        two = host(world, res_b, mode, seed=seed_b, into=host(world, res_a, mode))
        s1, s2 = one.summary(), two.summary()
        cu.assert_equal(s2, s1, f"mode {mode}")
        assert s2["batches"] == 2 and s1["batches"] == 1
        for t, n in enumerate(LENGTHS):
            assert np.array_equal(one.depth(t, 0, n), two.depth(t, 0, n))


@pytest.mark.parametrize("segment", ["64", "1000", None])
def test_the_segment_size_does_not_show(world, mapped, monkeypatch, segment):
    _, res, recs = mapped
    if segment is None:
        monkeypatch.delenv("MAPAD_COVERAGE_SEGMENT", raising=False)
    else:
        monkeypatch.setenv("MAPAD_COVERAGE_SEGMENT", segment)
    for mode in (1, 2):
        cu.assert_equal(host(world, res, mode).summary(), cu.from_records(LENGTHS, recs, mode), f"segment {segment}, mode {mode}")


def test_the_boundary(world):
    L = mapad_amd.lib()
    names = ("mapad_ctx_set_coverage", "mapad_ctx_coverage", "mapad_ctx_coverage_depth", "mapad_ctx_coverage_reset", "mapad_ctx_coverage_merge", "mapad_coverage_host_new",
             "mapad_coverage_host_add", "mapad_coverage_host_summary", "mapad_coverage_host_depth", "mapad_coverage_host_free")
    for name in names:
        assert name in mb.SYMBOLS and hasattr(L, name)
    for name in ("set_coverage", "coverage", "coverage_depth", "reset_coverage", "merge_coverage"):
        assert hasattr(mapad_amd.Context, name)
    assert mapad_amd.CoverageHost is mb.CoverageHost
    out = mb.CoverageC()
    assert C.sizeof(mb.CoverageContigC) == 5 * 8 and C.sizeof(out) == 8 + 8 + 256 * 8 + 6 * 8 + 2 * 8
    buf = (C.c_uint32 * 4)()
    assert L.mapad_ctx_set_coverage(None, 1) == -1 and L.mapad_ctx_coverage(None, C.byref(out)) == -1 and L.mapad_ctx_coverage_reset(None) == -1  # MAPAD_ERR_INVALID
    assert L.mapad_ctx_coverage_depth(None, 0, 0, 4, buf) == -1 and L.mapad_ctx_coverage_merge(None, None) == -1
    h = C.c_void_p()
    assert L.mapad_coverage_host_new(None, 1, C.byref(h)) == -1 and L.mapad_coverage_host_add(None, None, None, None, 0) == -1
    assert L.mapad_coverage_host_summary(None, C.byref(out)) == -1 and L.mapad_coverage_host_depth(None, 0, 0, 4, buf) == -1
    L.mapad_coverage_host_free(None)
    _, idx, _ = world
    with pytest.raises(mapad_amd.MapadError):  # mode 0 is not a host mode
        mb.CoverageHost(idx, 0)
    acc = mb.CoverageHost(idx, 1)
    with pytest.raises(mapad_amd.MapadError):  # a window that leaves its contig
        acc.depth(0, LENGTHS[0] - 3, 4)
    with pytest.raises(mapad_amd.MapadError):
        acc.depth(2, 0, 1)
    zero = acc.summary()
    assert zero["reads_seen"] == 0 and zero["batches"] == 0 and int(zero["hist"][0]) == sum(LENGTHS) and not zero["hist"][1:].any()
