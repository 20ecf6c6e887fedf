"""Duplicate collapsing on the GPU (run with -m gpu on an MI355X): with mapad_ctx_set_collapse_duplicates on, everything a caller can fetch is bit-identical to what it
fetches with it off — and the work of the duplicates was really skipped (mapad_last_collapse_info).  Batches come from synth.genome / synth.reads with reads
replicated by numpy (fixed seeds, shuffled so that copies are not neighbours)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import build as mbuild
from mapad_amd import synth
from oracle import binding as ob

from bam_util import read_bam
from kat_util import resolve_params
from parity_util import DAMAGE, IGNORE_BQ, NO_DAMAGE, assert_same_as_oracle, canonical_records, records_digest, split_reads

pytestmark = pytest.mark.gpu

DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)


def take(batch, idx):
    """the reads idx (in that order) of a batch -> a new batch"""
    seqs, quals, offsets = batch
    off = offsets.astype(np.int64)
    lens = (off[1:] - off[:-1])[idx]
    new_off = np.zeros(len(idx) + 1, np.uint64)
    new_off[1:] = np.cumsum(lens)
    first = np.cumsum(lens) - lens
    src = np.repeat(off[:-1][idx] - first, lens) + np.arange(int(lens.sum()), dtype=np.int64)
    return seqs[src], quals[src], new_off


def with_duplicates(batch, n_copies, seed):
    """the batch plus n_copies reads drawn from it again, shuffled"""
    n = len(batch[2]) - 1
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = np.concatenate([np.arange(n), rng.integers(0, n, n_copies)])
    return take(batch, rng.permutation(idx))


def twice(batch, seed):
    n = len(batch[2]) - 1
    return take(batch, np.random.Generator(np.random.PCG64(seed)).permutation(np.concatenate([np.arange(n), np.arange(n)])))


def numpy_groups(batch, ignore_qual=False):
    """(dup_of with the lowest index as representative, number of groups, reads that have a twin) by a dictionary of (length, bases, qualities)"""
    seqs, quals, offsets = batch
    n = len(offsets) - 1
    first, dup_of = {}, np.zeros(n, np.int64)
    for i in range(n):
        a, b = int(offsets[i]), int(offsets[i + 1])
        dup_of[i] = first.setdefault((seqs[a:b].tobytes(), b"" if ignore_qual else quals[a:b].tobytes()), i)
    sizes = np.bincount(dup_of, minlength=max(n, 1))
    return dup_of, len(first), int(sizes[sizes >= 2].sum())


def run(index, params, batch, collapse, tail_pops=None, fetch_d=True):
    """-> (result, collapse_info, tail_info) of one mapad_map_batch"""
    ctx = mapad_amd.Context(index, params, 0)
    try:
        ctx.set_collapse_duplicates(collapse)
        if tail_pops is not None:
            ctx.set_tail_pops(tail_pops)
        ctx.set_fetch_d_arrays(fetch_d)
        res = ctx.map_batch(*batch)
        return res, ctx.collapse_info(), ctx.tail_info()
    finally:
        ctx.close()


def assert_identical(a, b, offsets, d_arrays=True):
    """the raw arrays of two results"""
    assert a.n_reads == b.n_reads and a.n_hits == b.n_hits and a.n_ops == b.n_ops
    assert np.array_equal(a.hit_begin, b.hit_begin)
    for f in a.hits_arr.dtype.names:
        v, w = a.hits_arr[f], b.hits_arr[f]
        assert np.array_equal(v.view(np.uint32) if v.dtype == np.float32 else v, w.view(np.uint32) if w.dtype == np.float32 else w), f
    assert np.array_equal(a.ops, b.ops) and np.array_equal(a.status, b.status) and np.array_equal(a.counters, b.counters)
    if d_arrays:
        assert np.array_equal(a.d_arrays(offsets).view(np.uint32), b.d_arrays(offsets).view(np.uint32))


@pytest.fixture(scope="module")
def genome2m():
    g = synth.genome(2_000_000, seed=606)
    return g, mapad_amd.Index.build([("chr1", g)], device=0)


PRESETS = {"no_damage": (NO_DAMAGE, dict(qual=40)), "damage": (DAMAGE, dict(qual_range=(20, 23), damage=DMG)), "ignore_bq": (IGNORE_BQ, dict(qual_range=(2, 40), damage=DMG))}


@pytest.mark.parametrize("name", list(PRESETS))
def test_on_equals_off_bit_for_bit(genome2m, name):
    g, pidx = genome2m
    prm, kw = PRESETS[name]
    batch = with_duplicates(synth.reads(g, 24_000, 50, seed=11 + len(name), **kw), 16_000, seed=3)
    params = mapad_amd.make_params(resolve_params(prm))
    on, info, _ = run(pidx, params, batch, True)
    off, info_off, _ = run(pidx, params, batch, False)
    assert_identical(on, off, batch[2])
    n = len(batch[2]) - 1
    dup_of, groups, twins = numpy_groups(batch, ignore_qual=bool(prm["ignore_base_quality"]))  # (two reads from one place may differ in their qualities alone)
    assert info[0] == n and info[1] == groups < n and info[2] == twins and info[3] == 0 and info[7] == 0
    assert info[4] == int(off.counters["n_pop"][dup_of == np.arange(n)].sum())  # the pops of the representatives, and no others
    assert info_off == [n, n, 0, 0, 0, 0, 0, 0]  # off is off


def test_collapsed_result_equals_the_oracle(genome2m):
    g, pidx = genome2m
    batch = with_duplicates(synth.reads(g, 12_000, 50, seed=21, qual_range=(20, 23), damage=DMG), 8_000, seed=4)
    rp = resolve_params(DAMAGE)
    res, info, _ = run(pidx, mapad_amd.make_params(rp), batch, True)
    assert info[1] == numpy_groups(batch)[1] < info[0] == 20_000
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    reads, qs = split_reads(*batch)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=16, keep_d=True)
    assert_same_as_oracle(ores, res, batch[2], check_d=True, check_counters=True)


def test_a_batch_that_is_a_set_twice_searches_the_set_once(genome2m):
    g, pidx = genome2m
    u = synth.reads(g, 20_000, 50, seed=31, qual_range=(20, 40), damage=DMG)
    assert numpy_groups(u)[1] == 20_000  # no duplicate at this size (1 M reads on 48 Mbp do hold a few hundred)
    b = twice(u, seed=5)
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    on_b, info_b, _ = run(pidx, params, b, True, fetch_d=False)
    on_u, info_u, _ = run(pidx, params, u, True, fetch_d=False)
    off_u, _, _ = run(pidx, params, u, False, fetch_d=False)
    assert info_b[:4] == [40_000, 20_000, 40_000, 0] and info_u[:4] == [20_000, 20_000, 0, 0]
    assert info_b[4] == info_u[4] == int(off_u.counters["n_pop"].sum())
    assert int(on_b.counters["n_pop"].sum()) == 2 * info_b[4]  # what is fetched stands for every read
    assert_identical(on_u, off_u, u[2], d_arrays=False)
    assert on_b.n_hits == 2 * off_u.n_hits and on_b.n_ops == 2 * off_u.n_ops


def test_qualities_count_unless_they_are_ignored(genome2m):
    g, pidx = genome2m
    u = synth.reads(g, 3000, 50, seed=41, qual=30, damage=DMG)
    seqs, quals, offsets = twice(u, seed=6)
    dup_of, _, _ = numpy_groups((seqs, quals, offsets))
    second = np.flatnonzero(dup_of != np.arange(6000))
    quals = quals.copy()
    quals[offsets[second].astype(np.int64) + 7] = 31  # the second copy of every read differs in one quality
    batch = (seqs, quals, offsets)
    for prm, collapsed in ((DAMAGE, False), (IGNORE_BQ, True)):
        params = mapad_amd.make_params(resolve_params(prm))
        on, info, _ = run(pidx, params, batch, True)
        off, _, _ = run(pidx, params, batch, False)
        assert info[:3] == ([6000, 3000, 6000] if collapsed else [6000, 6000, 0]), prm
        assert_identical(on, off, offsets)


def _corner_batch():
    g = synth.genome(100_000, seed=5)
    g[40_000:40_400] = g[10_000:10_400]
    g[80_000:80_400] = g[10_000:10_400]
    parts = [synth.reads(g, 600, 50, seed=11), synth.reads(g, 300, 50, seed=12, indel_frac=0.6, exo_frac=0.0), synth.reads(g[10_000:10_400], 60, 50, seed=78, exo_frac=0.0)]
    seqs = np.concatenate([p[0] for p in parts])
    quals = np.concatenate([p[1] for p in parts])
    offsets = np.arange(0, 50 * 960 + 1, 50, dtype=np.uint64)
    return g, (seqs, quals, offsets)


def test_the_corners_of_the_result(monkeypatch):
    """Every read past the budget leaves for the host, whatever it has waiting (_corners)."""
    _corners(monkeypatch, "unconditional")


@pytest.mark.parametrize("gate", ["default"])
def test_the_corners_of_the_result_under_the_shipped_gate(monkeypatch, gate):
    _corners(monkeypatch, gate)


def _corners(monkeypatch, gate):
    """Duplicates of an unmapped read, a read with several hits, a gapped alignment, a read stopped by the search limits (status 2) and reads a host thread finishes.
    unconditional: every read past the budget leaves for the host, whatever it has waiting; default: the shipped gate (8 waiting reads per worker), under which the
    host's pace decides how many of them leave — between one (the first ask of a launch finds the ring empty and the pool idle) and all of them."""
    if gate == "unconditional":
        monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", "4294967295")  # every read past the budget leaves for the host, whatever it has waiting
    else:
        monkeypatch.delenv("MAPAD_TAIL_BACKLOG_BUDGET", raising=False)
    g, u = _corner_batch()
    batch = twice(u, seed=7)
    pidx = mapad_amd.Index.build([("chr1", g)])
    rp = dict(resolve_params(NO_DAMAGE), stack_limit=400, edit_tree_limit=100000, stack_limit_abort=1)  # (stops a dozen of the 960 reads)
    params = mapad_amd.make_params(rp)
    on, info, tail_on = run(pidx, params, batch, True, tail_pops=300)
    off, _, tail_off = run(pidx, params, batch, False, tail_pops=300)
    assert_identical(on, off, batch[2])
    assert info[:3] == [1920, 960, 1920]
    counts = np.diff(off.hit_begin.astype(np.int64))
    assert ((counts == 0) & (off.status == 0)).any() and (counts > 1).any() and (off.status == 2).any()
    assert (((off.ops >> 24) == 0) | ((off.ops >> 24) == 1)).any()  # an insertion or a deletion in an edit track
    if gate == "unconditional":
        assert tail_on["reads"] > 0 and tail_off["reads"] == 2 * tail_on["reads"]  # only representatives can be handed over
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    reads, qs = split_reads(*batch)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=16, keep_d=True)
    assert_same_as_oracle(ores, on, batch[2])
    pops = ores.counters[:, 3]
    past = int((pops > 300).sum())  # every read is in the batch twice: half of them are representatives
    assert past >= 2 and past % 2 == 0
    assert (on.status & 16).sum() == 0 and (off.status & 16).sum() == 0
    if gate == "unconditional":
        assert tail_off["reads"] == past
    else:
        for info, n_past in ((tail_on, past // 2), (tail_off, past)):
            assert 0 < info["reads"] <= n_past, (info, n_past)
            assert info["continued"] <= info["handed_over_with_state"] <= info["reads"] and info["gpu_pops"] >= 300 * (info["reads"] - info["reads_dry_class"] - info["reads_full_limit"]), info
        assert tail_on["host_pops"] <= int(pops[pops > 300].sum()) // 2 and tail_off["host_pops"] <= int(pops[pops > 300].sum())


@pytest.mark.parametrize("env", [{"MAPAD_ORDER": "0"}, {"MAPAD_HIT_POOL": "64"}, {"MAPAD_LANES_PER_READ": "2"}, {"MAPAD_ORDER_CHUNK_LOG2": "10"}], ids=["input_order", "hit_pool_overflow_retry", "pairs", "order_chunks_of_1024"])
def test_collapsing_under_the_scheduling_variants(genome2m, env, monkeypatch):
    """MAPAD_ORDER=0 leaves the search without a cost-class order: with collapsing on it still walks a list of representatives."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, pidx = genome2m
    batch = with_duplicates(synth.reads(g, 5000, 50, seed=51, qual_range=(20, 23), damage=DMG), 4000, seed=8)
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    on, info, _ = run(pidx, params, batch, True)
    monkeypatch.delenv("MAPAD_HIT_POOL", raising=False)
    off, _, _ = run(pidx, params, batch, False)
    assert_identical(on, off, batch[2])
    assert info[1] == numpy_groups(batch)[1] and info[2] == numpy_groups(batch)[2]


def _hip():
    mapad_amd.lib()
    paths = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln})
    return C.CDLL(paths[0] if paths else "libamdhip64.so")


def test_every_entry_path(genome2m):
    g, pidx = genome2m
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    b0 = with_duplicates(synth.reads(g, 9000, 50, seed=61, qual_range=(20, 23), damage=DMG), 6000, seed=9)
    b1 = twice(synth.reads(g, 4000, 50, seed=62, qual_range=(20, 23), damage=DMG), seed=10)
    want = [run(pidx, params, b, False)[0] for b in (b0, b1)]
    # submit + select + fetch, two batches in flight
    ctx = mapad_amd.Context(pidx, params, 0)
    try:
        ctx.set_pipeline_depth(2)
        ctx.set_collapse_duplicates(True)
        ctx.submit_batch(*b0)
        ctx.submit_batch(*b1)
        for age, b, w in ((1, b0, want[0]), (0, b1, want[1])):
            ctx.select_batch(age)
            assert_identical(ctx.fetch(), w, b[2])
            info = ctx.collapse_info()
            _, groups, twins = numpy_groups(b)
            assert info[:4] == [len(b[2]) - 1, groups, twins, 0] and info[4] > 0
        ctx.set_collapse_duplicates(False)  # waits for the batches in flight; the next batch is mapped read by read
        ctx.submit_batch(*b1)
        assert_identical(ctx.fetch(), want[1], b1[2])
        assert ctx.collapse_info() == [8000, 8000, 0, 0, 0, 0, 0, 0]
    finally:
        ctx.close()
    # device-resident inputs + the collect on the device
    hip = _hip()

    def to_device(a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 8))) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        return p.value

    def to_host(p, dtype, n):
        out = np.zeros(n, dtype)
        if n:
            assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(out.nbytes), 2) == 0
        return out

    dev = [to_device(a) for a in b0]
    got = {}
    for collapse in (True, False):
        ctx = mapad_amd.Context(pidx, params, 0)
        try:
            ctx.set_collapse_duplicates(collapse)
            ctx.prepare_lengths([50])
            ctx.map_batch_device(dev[0], dev[1], dev[2], len(b0[2]) - 1, 50)
            d_begin, d_hits, d_ops, n_hits, n_ops = ctx.compact_device()
            assert hip.hipDeviceSynchronize() == 0
            got[collapse] = (to_host(d_begin, np.uint64, len(b0[2])), to_host(d_hits, mapad_amd.binding.HIT_DTYPE, n_hits), to_host(d_ops, np.uint32, n_ops), ctx.collapse_info())
        finally:
            ctx.close()
    for p in dev:
        hip.hipFree(C.c_void_p(p))
    for k in range(3):
        assert np.array_equal(got[True][k].view(np.uint8), got[False][k].view(np.uint8))
    assert np.array_equal(got[True][0], want[0].hit_begin) and np.array_equal(got[True][2], want[0].ops)
    assert got[True][3][:4] == [15_000, numpy_groups(b0)[1], numpy_groups(b0)[2], 0] and got[False][3] == [15_000, 15_000, 0, 0, 0, 0, 0, 0]


def test_records_of_collapsed_and_uncollapsed_results_are_equal():
    g = synth.genome(120_000, seed=21)
    g[40_000:40_400] = g[10_000:10_400]  # repeats, so that multi-mapping (X0 > 1, XA, rows drawn from >= 3-row intervals) occurs
    g[80_000:80_400] = g[10_000:10_400]
    pidx = mapad_amd.Index.build([("c1", g[:50_000]), ("c2", g[50_000:90_000]), ("c3", g[90_000:])])
    seqs, quals, offsets = synth.reads(g, 300, 50, seed=77)
    rep = synth.reads(g[10_000:10_400], 60, 50, seed=78, exo_frac=0.0)
    u = (np.concatenate([seqs, rep[0]]), np.concatenate([quals, rep[1]]), np.concatenate([offsets, rep[2][1:] + offsets[-1]]))
    batch = with_duplicates(u, 400, seed=12)
    params = mapad_amd.make_params(resolve_params(NO_DAMAGE))
    digests, recs_of = {}, {}
    for collapse in (True, False):
        ctx = mapad_amd.Context(pidx, params, 0)
        try:
            ctx.set_collapse_duplicates(collapse)
            res = ctx.map_batch(*batch)
            recs, text = ctx.hits_to_records(res, *batch, seed=0, as_arrays=True)
            digests[collapse] = records_digest(canonical_records(recs, text, oracle_side=False))
            recs_of[collapse] = recs
        finally:
            ctx.close()
    assert digests[True] == digests[False]
    dup_of, _, _ = numpy_groups(batch)
    is_dup = dup_of != np.arange(len(dup_of))
    assert int(((recs_of[True]["x0"] > 1) & (recs_of[True]["mapped"] != 0) & is_dup).sum()) > 10  # every read draws its own stand-in for rand::rng(): exercised


def _decoded(path):
    text, refs, recs = read_bam(path)
    out = []
    for r in recs:
        tags = {k: v for k, v in r["tags"].items() if k != "XD"}  # (XD: wall time per read)
        out.append((r["name"], r["flags"], r["tid"], r["pos"], r["mapq"], r["cigar"], r["seq"], r["qual"], tuple(sorted(tags.items())), tuple(x for x in r["tag_order"] if x != "XD")))
    return refs, out


def test_cli_flag_writes_the_same_bam(tmp_path):
    mapad_amd.lib()
    cli = mbuild.build_cli()
    g = synth.genome(120_000, seed=17)
    fa, fq = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fastq")
    with open(fa, "w") as f:
        f.write(">chr1\n")
        s = g.tobytes().decode()
        for i in range(0, len(s), 60):
            f.write(s[i:i + 60] + "\n")
    seqs, quals, offsets = with_duplicates(synth.reads(g, 3000, 50, seed=23, qual_range=(20, 23), damage=DMG, len_range=(30, 80)), 2500, seed=13)
    with open(fq, "w") as f:
        for i in range(len(offsets) - 1):
            s, e = int(offsets[i]), int(offsets[i + 1])
            f.write(f"@r{i}\n{seqs[s:e].tobytes().decode()}\n+\n{''.join(chr(33 + q) for q in quals[s:e])}\n")
    subprocess.check_call([cli, "index", "-g", fa])
    base = [cli, "map", "-r", fq, "-g", fa, "-l", "single_stranded", "-p", "0.03", "-f", "0.5", "-t", "0.5", "-d", "0.02", "-s", "1.0", "-i", "0.001", "--seed", "7", "--batch_size", "2000"]
    subprocess.check_call(base + ["-o", str(tmp_path / "off.bam")])
    pr = subprocess.run(base + ["-o", str(tmp_path / "on.bam"), "--collapse_duplicates"], check=True, stderr=subprocess.PIPE, text=True)
    assert "duplicate collapsing: 5500 reads" in pr.stderr, pr.stderr
    off, on = _decoded(str(tmp_path / "off.bam")), _decoded(str(tmp_path / "on.bam"))
    assert len(on[1]) == 5500 and on == off
