"""The device-resident calls that bench.py and the one-process-per-GPU driver ship — mapad_ctx_set_stream + mapad_map_batch_device + mapad_compact_result_device /
mapad_records_device, mapad_device_result_ptrs, mapad_ctx_set_reserved_cus — held to the CPU oracle on a stream of the caller's own (run with -m gpu on an MI355X):

  a, b  inputs written by work that is still queued on the caller's stream when the batch is submitted are the inputs that are mapped (depths 1, 2, 3);
  c     a consumer queued on the caller's stream before a batch slot is launched again still reads its own batch;
  d     the device-side collect is ordered in front of what the caller queues behind mapad_compact_result_device;
  e, f  what mapad_records_device leaves for the multi-GPU gather — 88-byte records, text pool, pair pool — decodes to the oracle's records, as one batch and as
        shards under mapad_records_seed_at merged by merge_gathered_records, and through the overflow rerun of its per-slot pools;
  g     mapad_device_result_ptrs' raw pools before the collect;
  h     the accumulator stages reading the CALLER's input buffers at conversion time;
  i     CU-masked slot streams (mapad_ctx_set_reserved_cus), each configuration in a child process under a time limit of its own.

The delay (device_util.Hip.delay) is a host function that sleeps DELAY seconds on the caller's stream: a, b and c hold the stream with it, so that what they race
against (a whole submission, milliseconds) is over long before the stream moves on.  Measured on an MI355X: the undelayed sequence of case a — upload, submission,
fetch — takes 51 to 58 ms at depths 1, 2 and 3 (seven repetitions each; UNDELAYED_MS is the largest); DELAY = max(0.2 s, 20 x that) = 1.2 s.  Flags and MAPQ are not in the gather payload and are left out of e and f (device_util)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__" and ROOT not in sys.path:  # the reserved-CU child
    sys.path.insert(0, ROOT)

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import synth
from mapad_amd.distributed import merge_gathered_records
from oracle import binding as ob

import damage_util
import device_util as du
import records_util as ru
from kat_util import resolve_params
from parity_util import DAMAGE, _gather, assert_same_as_oracle, canonical_records, compare_records, split_reads

pytestmark = pytest.mark.gpu

UNDELAYED_MS = 58.0  # case a without its delay: upload, submission, fetch (the largest of the measured figures)
DELAY = max(0.2, 1.2)  # seconds: max(0.2, 20 * UNDELAYED_MS / 1000 rounded up)
assert DELAY >= 20 * UNDELAYED_MS / 1000
DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
N_READS = 2_000
D_READS = 100_000   # case d
BIG = 50_000        # case i: more reads than the resident wavefronts of every CU hold at once (16 reads per wavefront)
INVALID = -1        # MAPAD_ERR_INVALID


class World:
    """a 300 kbp synth.genome under the DAMAGE preset; batches of 50-base reads by seed, and the oracle's result of each (computed once)"""

    def __init__(self):
        self.g = synth.genome(300_000, seed=61)
        self.rp = resolve_params(DAMAGE)
        self.pidx = mapad_amd.Index.build([("chr1", self.g)])
        self.oidx = ob.OracleIndex.from_bwt(self.pidx.bwt(), "$ACGTX", 128)
        self.params = mapad_amd.make_params(self.rp)
        self._oracle = {}

    def batch(self, seed, n=N_READS):
        return synth.reads(self.g, n, 50, seed=seed, qual_range=(20, 40), damage=DMG)

    def oracle(self, seed, n=N_READS):
        if (seed, n) not in self._oracle:
            reads, qs = split_reads(*self.batch(seed, n))
            self._oracle[(seed, n)] = self.oidx.map_batch(ob.make_params(self.rp), reads, qs, n_threads=8, keep_d=True)
        return self._oracle[(seed, n)]

    def context(self, s, depth, reserve=(2 * N_READS, 100 * N_READS)):
        ctx = mapad_amd.Context(self.pidx, self.params, 0)
        ctx.set_stream(s)
        ctx.set_pipeline_depth(depth)
        ctx.prepare_lengths([50])
        if reserve:
            ctx.reserve(reserve[0], reserve[1], 50)  # no buffer is allocated, and none moves, inside a test's sequence
        return ctx


class OnDevice:
    """a batch's three input arrays in device buffers of the test's own"""

    def __init__(self, hip, batch):
        self.batch, self.n = batch, len(batch[2]) - 1
        self.ptrs = tuple(hip.to_device(a) for a in batch)
        self.max_len = int(np.diff(batch[2].astype(np.int64)).max()) if self.n else 0

    def submit(self, ctx):
        ctx.map_batch_device(self.ptrs[0], self.ptrs[1], self.ptrs[2], self.n, self.max_len)


@pytest.fixture(scope="module")
def hip():
    h = du.Hip()
    yield h
    h.release()


@pytest.fixture(scope="module")
def w(hip):
    return World()


@pytest.fixture
def s(hip):
    """a non-blocking stream of the test's own, destroyed behind it (a stream left alive keeps its share of the process's few hardware queues)"""
    stream = hip.stream()
    yield stream
    hip.destroy(stream)


def same_hits(res, ores):
    return np.array_equal(res.hit_begin, ores.hit_offsets) and np.array_equal(res.hits_arr["lower"], ores.intervals[:, 0])


# ---- a, b: inputs behind the caller's stream ----------------------------------------------------------------------------------------------------------------------
def overwritten_inputs_are_the_ones_mapped(hip, w, ctx, s, rounds):
    """The device buffers hold batch X; a delay and then the upload of batch Y (same lengths: a library that ignored the stream would map X, stale but valid reads)
    are queued on s; the batch is submitted while s is still held.  Once per batch slot, X and Y changing places: with few hardware queues one slot's stream may
    share its queue with s, and the runtime's own barrier then orders that slot whatever the library does."""
    seeds = (71, 72)
    assert np.array_equal(w.batch(71)[2], w.batch(72)[2])
    dev = OnDevice(hip, w.batch(seeds[0]))
    pin = {seed: [hip.pinned_copy(a) for a in w.batch(seed)] for seed in seeds}
    for r in range(rounds):
        stale, fresh = seeds[r % 2], seeds[(r + 1) % 2]
        hip.delay(s, DELAY)
        for p, a in zip(dev.ptrs, pin[fresh]):
            hip.copy_async(p, a.ctypes.data, a.nbytes, du.H2D, s)
        assert hip.busy(s)  # the reach condition: the upload has not happened when the library is called
        dev.submit(ctx)
        res = ctx.fetch()
        hip.synchronize(s)
        assert not same_hits(res, w.oracle(stale)), f"submission {r}: the reads that were in the buffers at submission were mapped, not the ones the caller's stream wrote"
        assert_same_as_oracle(w.oracle(fresh), res, w.batch(fresh)[2])


@pytest.mark.parametrize("depth", [2, 3])
def test_inputs_are_ordered_behind_the_callers_stream(hip, w, depth, s):
    """case a.  Measured on an MI355X: the undelayed sequence (upload, submission, fetch) takes 51 to 58 ms; the delay is 1.2 s."""
    ctx = w.context(s, depth)
    try:
        overwritten_inputs_are_the_ones_mapped(hip, w, ctx, s, rounds=depth)
    finally:
        ctx.close()


def test_depth_1_runs_on_the_callers_stream(hip, w, s):
    """case b: at depth 1 everything runs on s itself; then the host entry points with s set"""
    ctx = w.context(s, 1)
    try:
        overwritten_inputs_are_the_ones_mapped(hip, w, ctx, s, rounds=1)
        assert_same_as_oracle(w.oracle(71), ctx.map_batch(*w.batch(71)), w.batch(71)[2])
        hip.delay(s, DELAY / 4)  # the staging copies and the launch queue up behind it
        ctx.submit_batch(*w.batch(72))
        assert_same_as_oracle(w.oracle(72), ctx.fetch(), w.batch(72)[2])
    finally:
        ctx.close()


# ---- c: a consumer queued before the slot is launched again ---------------------------------------------------------------------------------------------------------
def test_a_consumer_queued_before_a_relaunch_reads_its_own_batch(hip, w, s):
    ctx = w.context(s, 2)
    try:
        k, k1, k2 = (OnDevice(hip, w.batch(seed)) for seed in (73, 74, 75))  # k + 2: different reads, no larger than k, in k's slot
        k.submit(ctx)
        p_begin, p_hits, p_ops, n_hits, n_ops = ctx.compact_device()
        want = ctx.fetch()
        assert (n_hits, n_ops) == (want.n_hits, want.n_ops) and n_hits > N_READS // 2
        out = hip.pinned(k.n + 1, np.uint64), hip.pinned(n_hits, mb.HIT_DTYPE), hip.pinned(n_ops, np.uint32)
        hip.delay(s, DELAY)
        for dst, src in zip(out, (p_begin, p_hits, p_ops)):
            hip.copy_async(dst.ctypes.data, src, dst.nbytes, du.D2H, s)
        assert hip.busy(s)
        k1.submit(ctx)
        k2.submit(ctx)
        again = ctx.compact_device()  # k + 2's collect, into the arrays the copies read
        assert again[:3] == (p_begin, p_hits, p_ops), "the slot's arrays moved: the case no longer shows anything"
        got2 = ctx.fetch()
        ctx.select_batch(1)
        got1 = ctx.fetch()
        hip.synchronize(s)
        assert not same_hits(got2, w.oracle(73))
        assert out[0].tobytes() == want.hit_begin.tobytes() and out[1].tobytes() == want.hits_arr.tobytes() and out[2].tobytes() == want.ops.tobytes(), \
            "the copies queued before the relaunch did not read batch k"
        assert_same_as_oracle(w.oracle(73), want, k.batch[2])
        assert_same_as_oracle(w.oracle(74), got1, k1.batch[2])
        assert_same_as_oracle(w.oracle(75), got2, k2.batch[2])
    finally:
        ctx.close()


# ---- d: the collect in front of the caller's stream -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collapse", [False, True], ids=["plain", "collapsed"])
def test_the_collect_is_ordered_in_front_of_the_callers_stream(hip, w, collapse, s):
    """case d: D2H copies queued on s directly behind mapad_compact_result_device, nothing synchronised but s, equal the later fetch.  D_READS reads in one batch;
    collapsed: a third of them copies of others, and the sizes returned are the expanded ones."""
    batch = damage_util.with_duplicates(w.batch(76, D_READS - D_READS // 3), D_READS // 3, seed=77) if collapse else w.batch(76, D_READS)
    n = len(batch[2]) - 1
    ctx = w.context(s, 2, reserve=(n, 50 * n))
    try:
        ctx.set_fetch_d_arrays(False)
        ctx.set_collapse_duplicates(collapse)
        dev = OnDevice(hip, batch)
        out = hip.pinned(n + 1, np.uint64), hip.pinned(3 * n, mb.HIT_DTYPE), hip.pinned(3 * 50 * n, np.uint32)  # (before the sequence: pinning takes milliseconds)
        dev.submit(ctx)
        p_begin, p_hits, p_ops, n_hits, n_ops = ctx.compact_device()
        hip.copy_async(out[0].ctypes.data, p_begin, 8 * (n + 1), du.D2H, s)
        hip.copy_async(out[1].ctypes.data, p_hits, 40 * min(n_hits, len(out[1])), du.D2H, s)
        hip.copy_async(out[2].ctypes.data, p_ops, 4 * min(n_ops, len(out[2])), du.D2H, s)
        hip.synchronize(s)
        assert n_hits <= len(out[1]) and n_ops <= len(out[2])
        got = out[0].copy(), out[1][:n_hits].copy(), out[2][:n_ops].copy()
        res = ctx.fetch()
        assert (res.n_reads, res.n_hits, res.n_ops) == (n, n_hits, n_ops) and n_hits > n // 2
        assert np.array_equal(got[0], res.hit_begin) and got[1].tobytes() == res.hits_arr.tobytes() and np.array_equal(got[2], res.ops)
        info = ctx.collapse_info()
        assert (info[1] < info[0] - n // 4) if collapse else (info[1] == info[0] == n), info
    finally:
        ctx.close()


# ---- e, f: the gather payload -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def a(hip):
    world, clean = ru.world_a()
    batch, straddlers = ru.reads_a(world, clean)
    return dict(world=world, clean=clean, batch=batch, straddlers=straddlers, dev=OnDevice(hip, batch), canon={})


def prepare(ctx, batch):
    ctx.prepare_lengths(sorted(set(np.diff(batch[2].astype(np.int64)).tolist())))


def payload(hip, ctx, n, seed):
    """mapad_records_device on the selected batch, its three arrays copied to the host as they are"""
    p_rec, p_text, p_pairs, text_bytes, n_pairs = ctx.records_device(seed=seed)
    return hip.from_device(p_rec, n * 22, np.int32), hip.from_device(p_text, text_bytes, np.uint8), hip.from_device(p_pairs, 2 * n_pairs, np.float32)


def canon_of(a, preset, res):
    """the oracle's records over the fetched hits of world A's whole batch (the search is deterministic: any fetch of that batch will do), computed once"""
    if preset not in a["canon"]:
        a["canon"][preset] = du.without_flags_and_mapq(a["world"].oracle_canon(preset, res, a["batch"]))
    return a["canon"][preset]


def check_payload(a, preset, arrays, res, batch, lo=0, hi=None, what=""):
    """decoded payload of reads [lo, hi) of world A's batch against the oracle's records over the fetched hits of the whole batch, and against the hit lists"""
    recs, text, extras = du.decode_device_records(*arrays)
    assert not extras["error"].any(), what
    n_bad, first, per_field = ru.differing((recs, text), a["canon"][preset], lo, hi)
    assert n_bad == 0, ru.report(first, per_field, what)
    assert du.check_payload_against_hits(res, batch[2], recs, extras)[0] == int((recs["mapped"] != 0).sum())
    return recs, text, extras


@pytest.mark.parametrize("preset", list(ru.PRESETS))
def test_the_gather_payload_is_the_records(hip, a, preset):
    """case e, one batch and shards.  The shards (device_util.shard_cuts): the reads in front of the batch's longest unmapped run in two shards, an empty shard, that run — a
    shard without a mapped read —, and the reads behind it; each converted under mapad_records_seed_at(seed, its first read)."""
    world, batch, dev = a["world"], a["batch"], a["dev"]
    n = dev.n
    ctx = mapad_amd.Context(world.pidx, ru.params(preset), 0)
    try:
        prepare(ctx, batch)
        dev.submit(ctx)
        whole = payload(hip, ctx, n, ru.SEED)
        res = ctx.fetch()
        canon_of(a, preset, res)
        recs, text, extras = check_payload(a, preset, whole, res, batch, what="one batch")
        ru.check_reach_a(ru.edge_counts_a(world, recs, text, a["straddlers"], res.hit_begin))
        assert sum(len(p) for p in extras["pairs"]) > 100
        # the same batch in shards
        cuts = du.shard_cuts(recs["mapped"] != 0)
        assert cuts[2][0] == cuts[2][1] and cuts[3][1] - cuts[3][0] >= 64 and cuts[-1][1] == n, cuts
        assert int((recs["x0"][cuts[1][0]:cuts[1][1]] >= 3).sum()) >= 100  # reads whose coordinate is drawn under the seed, in a shard that starts behind read 0
        parts = []
        for lo, hi in cuts:
            shard = OnDevice(hip, du.sub_batch(batch, lo, hi))
            shard.submit(ctx)
            parts.append(payload(hip, ctx, hi - lo, int(mapad_amd.lib().mapad_records_seed_at(ru.SEED, lo))))
        assert len(parts[2][0]) == 0 and not parts[3][0].reshape(-1, 22)[:, 3].any()
        m_recs, m_text, m_pairs, _ = merge_gathered_records([du.as_gather_parts(p) for p in parts])
        got = du.decode_device_records(m_recs, m_text, m_pairs)
        moved = np.flatnonzero((got[0]["pos"] != recs["pos"]) | (got[0]["tid"] != recs["tid"]))
        assert moved.size == 0, f"{moved.size} reads are reported elsewhere in shards than in one batch; their X0: {sorted(set(recs['x0'][moved].tolist()))[:10]}"
        n_bad, first, per_field = compare_records(canonical_records(*got[:2], oracle_side=False), canonical_records(recs, text, oracle_side=False))
        assert n_bad == 0, ru.report(first, per_field, "shards against one batch")
        check_payload(a, preset, (m_recs, m_text, m_pairs), res, batch, what="merged shards")
        assert int((recs["x0"][recs["mapped"] != 0] >= 3).sum()) >= ru.A_REACH["x0_ge_3"]  # reads whose coordinate is drawn under the seed
    finally:
        ctx.close()


def test_the_gather_payload_of_two_batches_in_flight(hip, a, s):
    """case e at depth 2: two batches in flight, converted oldest first through select_batch"""
    world, batch, dev = a["world"], a["batch"], a["dev"]
    preset = "damage"
    k = 600
    ctx = mapad_amd.Context(world.pidx, ru.params(preset), 0)
    try:
        ctx.set_stream(s)
        ctx.set_pipeline_depth(2)
        prepare(ctx, batch)
        head = OnDevice(hip, du.sub_batch(batch, 0, k))
        dev.submit(ctx)
        head.submit(ctx)
        ctx.select_batch(1)
        first = payload(hip, ctx, dev.n, ru.SEED)
        res = ctx.fetch()
        canon_of(a, preset, res)
        ctx.select_batch(0)
        second = payload(hip, ctx, k, ru.SEED)
        check_payload(a, preset, first, res, batch, what="the older batch")
        check_payload(a, preset, second, ctx.fetch(), head.batch, 0, k, what="the newer batch")
    finally:
        ctx.close()


def test_the_per_slot_pools_overflow_and_rerun(hip, a):
    """case f: a fresh context's first mapad_records_device call is a batch whose record text is more than twice the slot's first text pool (the batch is sized in
    tests/test_device_io_host.py): text_kernel runs, overflows, and runs again in a grown pool.  Then a small batch in the grown pool.  Only the text pool is
    covered: the pair pool starts at n + 2048 pairs, and no read of this world leaves more than a few (reads on the tandem repeat: a quarter of a pair each)."""
    world = a["world"]
    batch = du.repeat_batch(world, a["clean"], du.REPEAT_READS)
    n = du.REPEAT_READS
    ctx = mapad_amd.Context(world.pidx, ru.params("damage"), 0)
    try:
        prepare(ctx, batch)
        dev = OnDevice(hip, batch)
        dev.submit(ctx)
        p_rec, p_text, p_pairs, text_bytes, n_pairs = ctx.records_device(seed=ru.SEED)
        print(f"text bytes {text_bytes}, first pool {ru.initial_pools(n)[0]}")
        assert text_bytes > 2 * ru.initial_pools(n)[0]
        arrays = hip.from_device(p_rec, n * 22, np.int32), hip.from_device(p_text, text_bytes, np.uint8), hip.from_device(p_pairs, 2 * n_pairs, np.float32)
        res = ctx.fetch()
        ocanon = du.without_flags_and_mapq(world.oracle_canon("damage", res, batch))
        recs, text, extras = du.decode_device_records(*arrays)
        assert not extras["error"].any()
        n_bad, first, per_field = ru.differing((recs, text), ocanon)
        assert n_bad == 0, ru.report(first, per_field, "rerun")
        assert int(recs["cigar_len"].sum() + recs["md_len"].sum() + recs["xa_len"].sum()) == text_bytes
        du.check_payload_against_hits(res, batch[2], recs, extras)
        small = OnDevice(hip, du.sub_batch(batch, 0, 65))
        small.submit(ctx)
        recs, text, extras = du.decode_device_records(*payload(hip, ctx, 65, ru.SEED))
        n_bad, first, per_field = ru.differing((recs, text), ocanon, 0, 65)
        assert n_bad == 0 and not extras["error"].any(), ru.report(first, per_field, "in the grown pool")
    finally:
        ctx.close()


# ---- g: the raw pools ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_device_result_ptrs_before_the_collect(hip, w, s):
    """mapad_device_result_ptrs orders nothing: the stream is synchronised first.  Per read, hits_pool[hit_first[i] : + hit_count[i]] are its fetched hits."""
    ctx = w.context(s, 1)
    try:
        dev = OnDevice(hip, w.batch(78))
        dev.submit(ctx)
        hip.synchronize(s)
        p_count, p_first, p_pool, p_ops, p_cur = ctx.device_result_ptrs()
        count, first = hip.from_device(p_count, dev.n, np.uint32).astype(np.int64), hip.from_device(p_first, dev.n, np.uint32).astype(np.int64)
        n_hits, n_ops = (int(x) for x in hip.from_device(p_cur, 2, np.uint64))
        pool, ops_pool = hip.from_device(p_pool, n_hits, mb.HIT_DTYPE), hip.from_device(p_ops, n_ops, np.uint32)
        res = ctx.fetch()
        assert_same_as_oracle(w.oracle(78), res, dev.batch[2])
        assert (n_hits, n_ops) == (res.n_hits, res.n_ops) and n_hits > dev.n // 2
        assert np.array_equal(count, np.diff(res.hit_begin.astype(np.int64))) and (first + count <= n_hits).all()
        mine = _gather(pool, first, count)  # the pool's records in read order
        for k in ("lower", "lower_rev", "size", "n_ops"):
            assert np.array_equal(mine[k], res.hits_arr[k]), k
        assert np.array_equal(mine["score"].view(np.uint32), res.hits_arr["score"].view(np.uint32))
        assert (mine["ops_offset"].astype(np.int64) + mine["n_ops"] <= n_ops).all()
        assert np.array_equal(_gather(ops_pool, mine["ops_offset"], mine["n_ops"]), _gather(res.ops, res.hits_arr["ops_offset"], res.hits_arr["n_ops"]))
        assert np.array_equal(_gather(res.ops, res.hits_arr["ops_offset"], res.hits_arr["n_ops"]), res.ops)
    finally:
        ctx.close()


# ---- h: device inputs and the accumulator stages ------------------------------------------------------------------------------------------------------------------------
def test_the_stages_read_the_callers_buffers_at_conversion(hip, s):
    """case h: coverage, pileup and the damage score on; three batches at depth 2 on s through map_batch_device + records_device, the inputs left untouched until
    converted; summaries and windows equal the host accumulators' over the fetched results; a second conversion adds nothing"""
    from test_gpu_stages import LENGTHS, SPLIT, TOTAL, batches_of, canon, seed_at
    g = synth.genome(TOTAL, seed=83)
    g[7_000:7_200] = g[2_000:2_200]
    idx = mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batches = batches_of(g)
    ctx = mapad_amd.Context(idx, params, 0)
    cov, pil, dscore = mb.CoverageHost(idx, 1), mb.PileupHost(idx, 1), None
    windows = lambda f: [f(t, 0, n) for t, n in enumerate(LENGTHS)]  # noqa: E731
    reading = lambda: canon((ctx.damage_scores(), ctx.coverage(), windows(ctx.coverage_depth), ctx.pileup(), windows(ctx.pileup_counts)))  # noqa: E731
    try:
        ctx.set_stream(s)
        ctx.set_pipeline_depth(2)
        ctx.set_damage_score(1)
        ctx.set_coverage(1)
        ctx.set_pileup(1)
        for b in batches:
            prepare(ctx, b)
        devs = [OnDevice(hip, b) for b in batches]
        flying, todo, first = [], list(devs), 0
        while todo or flying:
            while todo and len(flying) < 2:
                todo[0].submit(ctx)
                flying.append(todo.pop(0))
            ctx.select_batch(len(flying) - 1)  # the oldest
            d = flying.pop(0)
            ctx.records_device(seed=seed_at(first))
            if not todo and not flying:
                before = reading()
                ctx.records_device(seed=seed_at(first))  # converted again: nothing is added
                assert reading() == before
            res = ctx.fetch()
            _, _, dscore = mb.damage_score_host(idx, params, res, *d.batch, seed=seed_at(first), into=dscore)
            cov.add(params, res, seed=seed_at(first))
            pil.add(params, res, *d.batch, seed=seed_at(first))
            first += d.n
        got = reading()
        want = canon((dscore, cov.summary(), windows(cov.depth), pil.summary(), windows(pil.counts)))
        assert got == want
        assert got[0]["reads_seen"] == got[1]["reads_seen"] == got[3]["reads_seen"] == first and got[1]["batches"] == 3
        assert got[0]["reads_scored"] > 0 and got[1]["covered_columns"] > 0 and got[3]["columns_counted"] > 0
    finally:
        ctx.close()


# ---- i: reserved CUs ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_reserved_cus_are_refused_where_they_cannot_hold(hip, w):
    """in this process, nothing launched under a CU mask: the argument checks of mapad_ctx_set_reserved_cus and of mapad_ctx_select_batch"""
    def code(fn, *args):
        with pytest.raises(mapad_amd.MapadError) as e:
            fn(*args)
        return e.value.code

    ctx = mapad_amd.Context(w.pidx, w.params, 0)
    try:
        assert code(ctx.set_reserved_cus, -1) == INVALID and code(ctx.set_reserved_cus, 1 << 20) == INVALID
        n_cu = next(n for n in range(1, 4097) if _refused(ctx, n))  # the first n that is refused is the device's CU count
        assert 64 <= n_cu <= 1024 and code(ctx.set_reserved_cus, n_cu) == INVALID and code(ctx.set_reserved_cus, n_cu + 1) == INVALID
        ctx.set_reserved_cus(n_cu - 1)
        ctx.set_reserved_cus(0)
        ctx.set_pipeline_depth(2)
        assert code(ctx.select_batch, 2) == INVALID and code(ctx.select_batch, -1) == INVALID
        ctx.prepare_lengths([50])
        ctx.reserve(64, 64 * 50, 50)  # the slots' streams exist from here on
        assert code(ctx.set_reserved_cus, 8) == INVALID and code(ctx.set_reserved_cus, 0) == INVALID
        assert code(ctx.select_batch, 2) == INVALID
    finally:
        ctx.close()


def _refused(ctx, n):
    try:
        ctx.set_reserved_cus(n)
        return False
    except mapad_amd.MapadError:
        return True


def reserved_child(n_cus):
    """(a process of its own) three batches of 3 000 reads back to back at depth 2 on a stream of the child's own, the slot streams under a CU mask that leaves
    n_cus CUs free: every batch equals the oracle's.  The reach condition — a search grid smaller than that of a context without the setting — cannot show on
    3 000 reads: their 188 wavefronts are fewer than any CU count allows (grid = min(wavefronts the reads fill, resident wavefronts of the CUs in use)).  A fourth
    batch of BIG reads fills the CUs: its grid is compared, and its fetched arrays equal those of the context without the setting."""
    hip = du.Hip()
    world = World()
    seeds = (81, 82, 83)
    big = OnDevice(hip, world.batch(84, BIG))
    grids, big_results = [], []
    for reserved in (0, n_cus):
        s = hip.stream()
        ctx = mapad_amd.Context(world.pidx, world.params, 0)
        ctx.set_stream(s)
        ctx.set_reserved_cus(reserved)  # before the depth, and so before any slot stream exists
        ctx.set_pipeline_depth(2)
        ctx.prepare_lengths([50])
        devs = [OnDevice(hip, world.batch(seed, 3_000)) for seed in (seeds if reserved else seeds[:1])]
        results, flying = [], []
        for d in devs:  # back to back: a batch is fetched only once its successor has been submitted, the way a chunk loop at depth 2 runs
            d.submit(ctx)
            flying.append(d)
            if len(flying) == 2:
                ctx.select_batch(1)
                results.append(ctx.fetch())
                flying.pop(0)
        ctx.select_batch(0)
        results.append(ctx.fetch())
        assert len(results) == len(devs)
        for seed, d, res in zip(seeds, devs, results):
            assert_same_as_oracle(world.oracle(seed, 3_000), res, d.batch[2])
        ctx.set_fetch_d_arrays(False)
        big.submit(ctx)
        res = ctx.fetch()
        grids.append(int(ctx.launch_info()[3]))
        big_results.append((res.hit_begin.tobytes(), res.hits_arr.tobytes(), res.ops.tobytes(), res.counters.tobytes()))
        assert res.n_hits > BIG // 2
        ctx.close()
    print(json.dumps({"reserved_cus": n_cus, "layout": os.environ.get("MAPAD_RESERVED_CU_LAYOUT"), "search_grid": grids}))
    assert 0 < grids[1] < grids[0], grids
    assert big_results[0] == big_results[1]
    hip.release()


_died = []  # the first child that failed or ran into its time limit: no further one is started


@pytest.mark.parametrize("n_cus,layout", [(8, None), (8, "striped"), (3, None)], ids=["8_blocked", "8_striped", "3_uneven"])
def test_reserved_cus_leave_the_results_alone(n_cus, layout):
    """case i: each configuration in a child process under a time limit of its own; a child that fails or hits its limit ends the case and starts nothing more"""
    if _died:
        pytest.fail(f"not started: an earlier child died ({_died[0]})")
    env = {k: v for k, v in os.environ.items() if k not in ("MAPAD_RESERVED_CU_LAYOUT", "MAPAD_RESERVED_CUS")}
    if layout:
        env["MAPAD_RESERVED_CU_LAYOUT"] = layout
    pr = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "reserved", str(n_cus)], env=env, cwd=ROOT,
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if pr.returncode != 0:
        _died.append(f"exit status {pr.returncode}: {n_cus} CUs, layout {layout}")
    assert pr.returncode == 0, pr.stdout[-3000:]
    line = json.loads([ln for ln in pr.stdout.splitlines() if ln.startswith("{")][-1])
    print(line)
    assert line["reserved_cus"] == n_cus and line["layout"] == layout and 0 < line["search_grid"][1] < line["search_grid"][0], line


if __name__ == "__main__":
    assert sys.argv[1] == "reserved"
    reserved_child(int(sys.argv[2]))
