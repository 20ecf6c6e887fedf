"""GPU tests of the host tail (csrc/host_tail.hpp): reads that pass a pop budget on the GPU are handed — by the running kernel, through page-locked
records — to the library's host threads, which map them from scratch with the kernel's own search step; their results join the batch before the
order-preserving collect.  Where a read was finished must not show anywhere: every result is compared bit for bit (hits, BinaryHeap order, score bits,
edit tracks, D arrays, the six event counters) with the CPU oracle and with the same batch mapped with the tail switched off.
Reference behaviour at stake: the overflow recovery of src/map/mapping.rs:1358-1380 (the reads that get here at the real limits are those that hit it)."""
import numpy as np
import pytest

import mapad_amd
from mapad_amd import synth
from oracle import binding as ob

import sweep_util as su
from kat_util import resolve_params
from parity_util import CONTINUOUS, DAMAGE, NO_DAMAGE, assert_same_as_oracle, split_reads

pytestmark = pytest.mark.gpu


GATES = {"unconditional": "4294967295", "default": None, "one_at_a_time": "1"}


@pytest.fixture(params=["unconditional", "default"])
def gate(request, monkeypatch):
    """The rule under which a read past the pop budget leaves (MAPAD_TAIL_BACKLOG_BUDGET; search_kernel: give_to_host).
    unconditional: whatever the host has waiting — round 5's atomicAdd hand-over; exactly the reads past the budget leave, and the counts are exact.
    default: the shipped gate — while fewer than 8 reads per worker wait or run, the ring slot claimed by CAS under that test.
    one_at_a_time: a limit of one — a read leaves only when no task waits or runs and the dispatcher has picked up every record of the launch.
    Under the two gated rules the host's pace decides how many reads leave (a refused read of these batches ends long before its second ask, 16 384 pops later): the
    counts become bounds (_gated_counts); where a read was finished still shows nowhere.  A test that needs all three asks for them with `_ALL_GATES`."""
    if GATES[request.param] is None:
        monkeypatch.delenv("MAPAD_TAIL_BACKLOG_BUDGET", raising=False)
    else:
        monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", GATES[request.param])
    return request.param


_ALL_GATES = pytest.mark.parametrize("gate", list(GATES), indirect=True)


@pytest.fixture
def _hand_over_whatever_the_backlog(monkeypatch):
    """For the tests that set their own gate (and start from round 5's rule, as they always have): every read past the budget leaves, whatever the host has waiting."""
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", "4294967295")


_own_gate = pytest.mark.usefixtures("_hand_over_whatever_the_backlog")


def _left_at_an_ask(info):
    """The reads that left at an ask point, with the budget's pops or more behind them.  The others left for a dry arena class or because no growable arena holds them
    (give_to_host's other two callers), at whatever pop count they had: with 32-node base arenas and a budget of 150 pops the classes beyond the budget keep four
    arenas each (launch_batch: MAPAD_BEYOND_BUDGET_ARENAS), and a read whose first hundred pops leave it with more than 512 nodes finds its class dry BEFORE its
    first ask.  Where nobody left for those reasons this is info["reads"]."""
    return info["reads"] - info["reads_dry_class"] - info["reads_full_limit"]


def _gated_counts(info, pops, budget, least=1):
    """What holds of a launch's tail counts under a gated rule, whatever the host's pace; `pops`: the oracle's pops per read.  Returns the number of reads past the budget.
    least = 1: the first ask of a launch whose process has no tail task waiting or running sees a backlog word of 0 (launch_batch: ctl[0] = pending()) and an empty
    ring (cursor == ctl[1] == 0), so it is granted under any limit >= 1.  A launch that starts while an earlier, uncollected launch still has tasks in the pool has no
    such promise (ctl[0] counts the tasks of all launches): least = 0 there."""
    past = int((pops > budget).sum())
    print("tail counts:", info, "past the budget:", past)
    assert least <= info["reads"] <= past, (info, past)  # only reads past the budget ask, each for one record
    assert info["continued"] <= info["handed_over_with_state"] <= info["reads"], info
    assert info["gpu_pops"] >= budget * _left_at_an_ask(info), info
    assert info["host_pops"] <= int(pops[pops > budget].sum()), info  # from scratch the host repeats a read's pops, continued it makes the rest of them
    return past


def _map(index, params, seqs, quals, offsets, tail_pops):
    ctx = mapad_amd.Context(index, params, 0)
    try:
        ctx.set_tail_pops(tail_pops)
        res = ctx.map_batch(seqs, quals, offsets)
        return res, ctx.tail_info()
    finally:
        ctx.close()


def _same(a, b):
    assert np.array_equal(a.hit_begin, b.hit_begin) and np.array_equal(a.hits_arr, b.hits_arr) and np.array_equal(a.ops, b.ops)
    assert np.array_equal(a.status, b.status) and np.array_equal(a.counters, b.counters)


@pytest.mark.parametrize("name,prm,kw,n", [
    ("no_damage", NO_DAMAGE, dict(qual=40), 3000),
    ("damage_mixed_len_indels", DAMAGE, dict(qual_range=(20, 40), len_range=(35, 100), indel_frac=0.05), 800),
    ("continuous_bound", CONTINUOUS, dict(qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0)), 2000),
])
def test_reads_finished_on_the_host_equal_the_oracle(name, prm, kw, n, gate):
    g = synth.genome(300_000, seed=77)
    seqs, quals, offsets = synth.reads(g, n, 50, seed=3 + len(name), **kw)
    rp = resolve_params(prm)
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    params = mapad_amd.make_params(rp)
    res, info = _map(pidx, params, seqs, quals, offsets, tail_pops=48)  # a budget most reads with a mismatch exceed
    reads, qs = split_reads(seqs, quals, offsets)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
    assert_same_as_oracle(ores, res, offsets)
    pops = ores.counters[:, 3]
    if gate == "unconditional":
        assert info["reads"] == int((pops > 48).sum()) > n // 20  # exactly the reads beyond the budget went to the host, and they are many
        assert info["host_pops"] == int(pops[pops > 48].sum()) and info["gpu_pops"] >= 48 * info["reads"]
    else:
        assert _gated_counts(info, pops, 48) > n // 20
    assert (res.status & 16).sum() == 0  # no read is left marked "handed over"
    off, info_off = _map(pidx, params, seqs, quals, offsets, tail_pops=0)
    assert info_off["reads"] == 0
    _same(res, off)


@_own_gate
def test_reads_past_the_budget_stay_on_the_gpu_while_the_host_is_busy(monkeypatch):
    """Round 6: every hand-over trigger looks at the host's backlog (the word the launch's dispatcher keeps current).  With no room at all
    (MAPAD_TAIL_BACKLOG_BUDGET=0) every read past the budget is refused, goes on on the GPU, asks again every 16 384 pops and finishes there; with the
    default (8 waiting reads per worker) any number between none and all of them leave, as the host's pace has it.  Nothing of that shows in the results."""
    g = synth.genome(300_000, seed=77)
    seqs, quals, offsets = synth.reads(g, 3000, 50, seed=12, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0))
    rp = resolve_params(DAMAGE)
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    params = mapad_amd.make_params(rp)
    reads, qs = split_reads(seqs, quals, offsets)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
    past = int((ores.counters[:, 3] > 64).sum())
    every, info_every = _map(pidx, params, seqs, quals, offsets, tail_pops=64)
    assert info_every["reads"] == past > 500
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", "0")
    res, info = _map(pidx, params, seqs, quals, offsets, tail_pops=64)
    assert info["reads"] == 0, info
    assert_same_as_oracle(ores, res, offsets)
    _same(res, every)
    assert (res.status & 16).sum() == 0
    monkeypatch.delenv("MAPAD_TAIL_BACKLOG_BUDGET")
    res, info = _map(pidx, params, seqs, quals, offsets, tail_pops=64)
    assert 0 <= info["reads"] <= past
    _same(res, every)


@_own_gate
def test_reads_below_the_budget_leave_while_a_worker_is_idle(monkeypatch):
    """Round 6: from MAPAD_TAIL_POPS_IDLE pops on a read leaves although it is short of the budget — while fewer reads than MAPAD_TAIL_BACKLOG_IDLE (default: the workers)
    wait or run on the host, i.e. while a worker is idle; the ring slot is claimed under that test (the kernel counts the records the dispatcher has not picked up yet
    itself), so the hundreds of reads that ask in the same microsecond cannot overrun it.  With no room (0) nobody leaves.  Nothing of that shows in the results."""
    g = synth.genome(300_000, seed=77)
    seqs, quals, offsets = synth.reads(g, 3000, 50, seed=12, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0))
    rp = resolve_params(DAMAGE)
    pidx = mapad_amd.Index.build([("chr1", g)])
    params = mapad_amd.make_params(rp)
    off, info_off = _map(pidx, params, seqs, quals, offsets, tail_pops=0)
    past = int((off.counters["n_pop"] > 64).sum())
    assert info_off["reads"] == 0 and past > 500
    monkeypatch.setenv("MAPAD_TAIL_POPS_IDLE", "64")
    res, info = _map(pidx, params, seqs, quals, offsets, tail_pops=1 << 20)  # a budget no read of this batch reaches
    assert 0 < info["reads"] == info["reads_idle_tier"] <= past, info
    assert info["gpu_pops"] >= 64 * info["reads"]
    _same(res, off)
    assert (res.status & 16).sum() == 0
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_IDLE", "0")
    res, info = _map(pidx, params, seqs, quals, offsets, tail_pops=1 << 20)
    assert info["reads"] == 0, info
    _same(res, off)
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_IDLE", "4294967295")  # whatever the backlog: every read past 64 pops
    res, info = _map(pidx, params, seqs, quals, offsets, tail_pops=1 << 20)
    assert info["reads"] == info["reads_idle_tier"] == past and info["gpu_pops"] == 64 * past, (info, past)  # each left at its first ask
    _same(res, off)


def test_limit_recovery_and_abort_on_the_host(gate):
    """Tiny STACK_LIMIT / EDIT_TREE_LIMIT: the reads that reach the host run into the overflow recovery (pop_min eviction, slab key reuse) or the abort there."""
    g = synth.genome(100_000, seed=5)
    seqs, quals, offsets = synth.reads(g, 600, 50, seed=11)
    reads, qs = split_reads(seqs, quals, offsets)
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    for limits in ({"stack_limit": 40, "edit_tree_limit": 100000}, {"stack_limit": 100000, "edit_tree_limit": 120}, {"stack_limit": 40, "edit_tree_limit": 100000, "stack_limit_abort": 1}):
        rp = dict(resolve_params(NO_DAMAGE), **limits)
        res, info = _map(pidx, mapad_amd.make_params(rp), seqs, quals, offsets, tail_pops=30)
        ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
        if gate == "unconditional":
            assert ores.counters[:, 3].max() > 40 and info["reads"] > 20
        else:
            assert ores.counters[:, 3].max() > 40 and _gated_counts(info, ores.counters[:, 3], 30) > 20
        assert_same_as_oracle(ores, res, offsets)
        if limits.get("stack_limit_abort"):
            assert (res.status == 2).any()


def test_full_ring_leaves_reads_on_the_gpu(monkeypatch, gate):
    """More reads pass the budget than the ring has records: the rest stays on the GPU; nothing changes."""
    monkeypatch.setenv("MAPAD_TAIL_RING", "16")
    g = synth.genome(200_000, seed=9)
    seqs, quals, offsets = synth.reads(g, 2000, 50, seed=2, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0))
    rp = resolve_params(DAMAGE)
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    res, info = _map(pidx, mapad_amd.make_params(rp), seqs, quals, offsets, tail_pops=40)
    reads, qs = split_reads(seqs, quals, offsets)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
    if gate == "unconditional":
        assert info["reads"] == 16 < int((ores.counters[:, 3] > 40).sum())
    else:
        assert info["reads"] <= 16 < _gated_counts(info, ores.counters[:, 3], 40)
    assert_same_as_oracle(ores, res, offsets)


def test_hit_pools_too_small_for_the_hosts_results_are_grown_and_the_batch_rerun(monkeypatch, gate):
    """The host's hits are appended to the batch's device pools; when they do not fit (here: pools of 64 hits), the collect reports it like a kernel-side overflow and
    mapad_map_batch re-runs the batch — GPU stages and host tail — with pools sized for everything."""
    monkeypatch.setenv("MAPAD_HIT_POOL", "64")
    g = synth.genome(200_000, seed=13)
    seqs, quals, offsets = synth.reads(g, 1500, 50, seed=4, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0))
    rp = resolve_params(DAMAGE)
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    res, info = _map(pidx, mapad_amd.make_params(rp), seqs, quals, offsets, tail_pops=40)
    reads, qs = split_reads(seqs, quals, offsets)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
    if gate == "unconditional":
        assert res.n_hits > 64 and info["reads"] == int((ores.counters[:, 3] > 40).sum()) > 50
    else:  # (the counts are the re-run's: the first run's tail is finished or cancelled before the batch is launched again)
        assert res.n_hits > 64 and _gated_counts(info, ores.counters[:, 3], 40) > 50
    assert_same_as_oracle(ores, res, offsets)


@_ALL_GATES
def test_tail_with_batches_in_flight_and_an_uncollected_batch(gate):
    """Three batches in flight, each with reads on the host; the collect of a batch waits for ITS host reads only.  A batch whose slot is reused before anybody
    collected it is dropped together with its host reads."""
    g = synth.genome(300_000, seed=31)
    rp = resolve_params(DAMAGE)
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    batches = [synth.reads(g, 1500, 50, seed=40 + i, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0)) for i in range(5)]
    ctx = mapad_amd.Context(pidx, mapad_amd.make_params(rp), 0)
    try:
        ctx.set_pipeline_depth(3)
        ctx.set_tail_pops(64)
        got = {}
        for i, b in enumerate(batches):
            ctx.submit_batch(*b)
            if i >= 2:
                ctx.select_batch(2)
                got[i - 2] = (ctx.fetch(), ctx.tail_info())
                ctx.select_batch(0)
        for age, i in ((1, 3), (0, 4)):
            ctx.select_batch(age)
            got[i] = (ctx.fetch(), ctx.tail_info())
        # two more batches are submitted and never collected; then the slots are reused
        for b in batches[:4]:
            ctx.submit_batch(*b)
        ctx.select_batch(0)
        again = ctx.fetch()
    finally:
        ctx.close()
    for i, b in enumerate(batches):
        reads, qs = split_reads(*b)
        ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
        assert_same_as_oracle(ores, got[i][0], b[2])
        if gate == "unconditional":
            assert got[i][1]["reads"] == int((ores.counters[:, 3] > 64).sum()) > 20
        else:  # only the context's first launch finds the pool idle for certain: the later ones start while their predecessors' reads wait or run on the host
            assert _gated_counts(got[i][1], ores.counters[:, 3], 64, least=1 if i == 0 else 0) > 20
        assert (got[i][0].status & 16).sum() == 0
    _same(again, got[3][0])


@_own_gate
def test_a_dry_arena_class_sends_reads_to_the_host(monkeypatch):
    """Round 5: a read that needs a grown arena of a scarce class while every one is taken asks for the host instead of queuing (DeviceGrow::acquire) — here every
    class counts as scarce, each has two arenas, and the pop budget is out of reach, so whatever goes to the host goes for that reason (or because no class holds it)."""
    monkeypatch.setenv("MAPAD_TIER0_NODES", "32")
    monkeypatch.setenv("MAPAD_CLASS_COUNTS", "2,2,2,2,2,2,2,2,2,2")
    monkeypatch.setenv("MAPAD_SET_ARENAS", "0")  # (idle sets of base arenas would take the reads the dry classes turn away: tests/test_gpu_parity.py covers those)
    monkeypatch.setenv("MAPAD_TAIL_MIN_CLASS", "0")
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG", "100000")  # the host takes whatever comes
    g = synth.genome(200_000, seed=21)
    seqs, quals, offsets = synth.reads(g, 4000, 50, seed=6, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0))
    rp = resolve_params(DAMAGE)
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    res, info = _map(pidx, mapad_amd.make_params(rp), seqs, quals, offsets, tail_pops=1 << 30)
    reads, qs = split_reads(seqs, quals, offsets)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
    assert_same_as_oracle(ores, res, offsets)
    assert info["reads_dry_class"] > 50 and info["reads"] == info["reads_dry_class"] + info["reads_full_limit"]
    assert (res.status & 16).sum() == 0
    # a backlog limit of zero: the host is "busy" from the start, nobody is handed over for a dry class; the reads queue on the GPU as in round 4
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG", "0")
    res0, info0 = _map(pidx, mapad_amd.make_params(rp), seqs, quals, offsets, tail_pops=1 << 30)
    assert info0["reads_dry_class"] == 0
    _same(res, res0)


@_own_gate
def test_reads_no_growable_arena_holds_go_to_the_host_instead_of_the_full_limit_stage(monkeypatch):
    """The classes end at 128 nodes: a read that needs more would be re-run by the full-limit stage (heavy_kernel, 336 MB arenas); with the host tail on it goes to a
    host thread.  n_third_pass counts such reads wherever they were finished; with the tail off the GPU's last stage takes them — same results."""
    monkeypatch.setenv("MAPAD_TIER0_NODES", "32")
    monkeypatch.setenv("MAPAD_CLASS_COUNTS", "512,512")
    monkeypatch.setenv("MAPAD_SET_ARENAS", "0")
    monkeypatch.setenv("MAPAD_TAIL_MIN_CLASS", "10")  # no hand-over for dry classes: only the reads no class can hold
    g = synth.genome(100_000, seed=5)
    seqs, quals, offsets = synth.reads(g, 1500, 50, seed=11)
    rp = resolve_params(NO_DAMAGE)
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    reads, qs = split_reads(seqs, quals, offsets)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
    res, info = _map(pidx, mapad_amd.make_params(rp), seqs, quals, offsets, tail_pops=1 << 30)
    assert_same_as_oracle(ores, res, offsets)
    assert info["reads_full_limit"] > 20 and info["reads"] == info["reads_full_limit"] == res.n_third_pass
    off, info_off = _map(pidx, mapad_amd.make_params(rp), seqs, quals, offsets, tail_pops=0)
    assert info_off["reads"] == 0 and off.n_third_pass == res.n_third_pass
    _same(res, off)


def test_hand_overs_reach_the_host_while_the_launch_is_running(gate):
    """The ring is host-coherent page-locked memory and every word of a record is written through (hand_to_host): the dispatcher thread sees records — and the
    workers start on them — during the launch, not when it ends (with ordinary page-locked memory that was luck)."""
    g = synth.genome(2_000_000, seed=41)
    seqs, quals, offsets = synth.reads(g, 400_000, 50, seed=8, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0))
    pidx = mapad_amd.Index.build([("chr1", g)], device=0)
    res, info = _map(pidx, mapad_amd.make_params(resolve_params(DAMAGE)), seqs, quals, offsets, tail_pops=4096)
    if gate == "unconditional":
        assert info["reads"] > 100, info
    else:  # (the first ask of the launch is granted: _gated_counts)
        assert info["reads"] > 0 and info["continued"] <= info["handed_over_with_state"] <= info["reads"] and info["gpu_pops"] >= 4096 * _left_at_an_ask(info), info
    assert info["seen_live"] > info["reads"] // 2, info  # the launch runs for a good 100 ms; the first hand-overs come within the first few
    assert (res.status & 16).sum() == 0


@pytest.mark.parametrize("name,prm,kw,n", [
    ("damage", DAMAGE, dict(qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0)), 3000),
    ("mixed_len_indels", DAMAGE, dict(qual_range=(20, 40), len_range=(35, 100), indel_frac=0.05), 800),
    ("continuous_bound", CONTINUOUS, dict(qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0)), 2000),
])
@_ALL_GATES
def test_reads_handed_over_with_their_search_are_continued_on_the_host(name, prm, kw, n, monkeypatch, gate):
    """Round 5: a read that sits in a grown arena when it is handed over leaves the arena to the host (heap top written out of LDS, SearchState in the record); a
    worker copies heap and nodes over PCIe, releases the arena and goes on where the GPU stopped (host_tail.hpp: TailState).  32-node base arenas make every read
    of consequence grow before the 150-pop budget; the results — event counters included, which now add GPU pops and host pops of one read — equal the oracle's
    and those of the same batch mapped from scratch on the host (MAPAD_TAIL_CONTINUE=0) and entirely on the GPU."""
    monkeypatch.setenv("MAPAD_TIER0_NODES", "32")
    g = synth.genome(300_000, seed=77)
    seqs, quals, offsets = synth.reads(g, n, 50, seed=3 + len(name), **kw)
    rp = resolve_params(prm)
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    params = mapad_amd.make_params(rp)
    res, info = _map(pidx, params, seqs, quals, offsets, tail_pops=150)
    reads, qs = split_reads(seqs, quals, offsets)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
    assert_same_as_oracle(ores, res, offsets)
    pops = ores.counters[:, 3]
    if gate == "unconditional":
        assert info["reads"] == int((pops > 150).sum()) > n // 50
        assert info["continued"] > info["reads"] // 2 and info["handed_over_with_state"] >= info["continued"], info  # (reads with a hit already found go from scratch)
        assert info["host_pops"] < int(pops[pops > 150].sum()) - 100 * info["continued"]  # the host did not repeat the GPU's pops of the continued reads
    else:
        assert _gated_counts(info, pops, 150) > n // 50
        assert info["host_pops"] <= int(pops[pops > 150].sum()) - 150 * info["continued"]  # (a continued read had made its 150 pops on the GPU)
    assert (res.status & 16).sum() == 0
    monkeypatch.setenv("MAPAD_TAIL_CONTINUE", "0")
    scratch, info0 = _map(pidx, params, seqs, quals, offsets, tail_pops=150)
    if gate == "unconditional":
        assert info0["continued"] == 0 and info0["reads"] == info["reads"]
    else:
        assert info0["continued"] == 0 and info0["handed_over_with_state"] == 0 and _gated_counts(info0, pops, 150)
    _same(res, scratch)
    off, _ = _map(pidx, params, seqs, quals, offsets, tail_pops=0)
    _same(res, off)


@_ALL_GATES
def test_arenas_of_reads_nobody_came_for_are_released(monkeypatch, gate):
    """Batches with reads handed over WITH their state are submitted and never collected; their slots are reused.  The grown arenas those reads still hold must go
    back to the pools (drop_tail): with two arenas per class a leak would leave later batches without any — they would still finish (dry classes send reads to
    the host) but with every class dry from the start, which the migration count shows."""
    monkeypatch.setenv("MAPAD_TIER0_NODES", "32")
    monkeypatch.setenv("MAPAD_CLASS_COUNTS", "8,8,8,8,8,8,8,8,8,8")
    monkeypatch.setenv("MAPAD_SET_ARENAS", "0")
    g = synth.genome(200_000, seed=31)
    rp = resolve_params(DAMAGE)
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    b = synth.reads(g, 1500, 50, seed=44, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0))
    ctx = mapad_amd.Context(pidx, mapad_amd.make_params(rp), 0)
    try:
        ctx.set_pipeline_depth(2)
        ctx.set_tail_pops(150)
        for _ in range(12):  # each submission reuses a slot whose batch nobody collected
            ctx.submit_batch(*b)
        ctx.select_batch(0)
        res = ctx.fetch()
        info = ctx.tail_info()
    finally:
        ctx.close()
    reads, qs = split_reads(*b)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
    assert_same_as_oracle(ores, res, b[2])
    assert info["handed_over_with_state"] > 0 and res.n_second_pass > 500  # reads still find grown arenas: nothing leaked
    assert info["continued"] <= info["handed_over_with_state"] <= info["reads"] and (res.status & 16).sum() == 0, info


@_ALL_GATES
def test_an_arena_relayout_waits_for_the_host_tails_of_uncollected_batches(monkeypatch, gate):
    """a batch with more reads than the arenas were laid out for makes the context free and re-allocate its pools.  Reads of ANOTHER slot's uncollected batch
    that were handed over with their state still own grown arenas in those pools until a host worker has copied them (and the workers read the pool descriptors
    unlocked): the re-layout first finishes and merges the host tails of every slot (finish_tails), and the earlier batch's results — collected afterwards — are
    still the oracle's."""
    monkeypatch.setenv("MAPAD_TIER0_NODES", "32")
    g = synth.genome(300_000, seed=77)
    rp = resolve_params(DAMAGE)
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    small = synth.reads(g, 1500, 50, seed=61, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0))
    big = synth.reads(g, 12_000, 50, seed=62, qual=40, subst_rate=0.0, exo_frac=0.0)  # (exact reads: a few dozen pops each, nothing for the host — the re-layout is what this batch is for)
    ctx = mapad_amd.Context(pidx, mapad_amd.make_params(rp), 0)
    try:
        ctx.set_pipeline_depth(2)
        ctx.set_tail_pops(150)
        ctx.submit_batch(*small)   # reads go to the host with their state; nobody collects yet
        ctx.submit_batch(*big)     # more reads than the pools were sized for: the arenas are laid out anew
        ctx.select_batch(1)
        first, info = ctx.fetch(), ctx.tail_info()
        ctx.select_batch(0)
        second = ctx.fetch()
    finally:
        ctx.close()
    if gate == "unconditional":
        assert info["handed_over_with_state"] > 50, info
    for b, res in ((small, first), (big, second)):
        reads, qs = split_reads(*b)
        ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
        assert_same_as_oracle(ores, res, b[2])
        assert (res.status & 16).sum() == 0
        if gate != "unconditional" and b is small:  # (the context's first launch)
            assert _gated_counts(info, ores.counters[:, 3], 150) > 50


@_ALL_GATES
def test_hand_over_ring_is_not_fooled_by_records_of_earlier_launches(gate):
    """the ring's `ready` words used to be cleared by count, and a small batch between two large ones left records of the first large batch marked ready when
    the third ran — the dispatcher would have taken a stale record for a new one.  A record is ready when its word holds THIS launch's number now.  Same context, same
    slot: 2 000 hand-overs, then a batch of 100 reads (ring of 100 records), then another large batch — every batch equals the oracle and hands over exactly its own reads."""
    g = synth.genome(300_000, seed=77)
    rp = resolve_params(NO_DAMAGE)
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    ctx = mapad_amd.Context(pidx, mapad_amd.make_params(rp), 0)
    try:
        ctx.set_tail_pops(48)
        for n, seed in ((3000, 71), (100, 72), (3000, 73), (100, 74), (2500, 75)):
            b = synth.reads(g, n, 50, seed=seed, qual=40)
            res = ctx.map_batch(*b)
            info = ctx.tail_info()
            reads, qs = split_reads(*b)
            ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
            assert_same_as_oracle(ores, res, b[2])
            if gate == "unconditional":
                assert info["reads"] == int((ores.counters[:, 3] > 48).sum()) and (res.status & 16).sum() == 0
            else:  # (every launch starts after the collect of the one before it: the pool is idle)
                assert _gated_counts(info, ores.counters[:, 3], 48) > 0 and (res.status & 16).sum() == 0
    finally:
        ctx.close()


# ---- round 6's gate at work: re-asks, a crowd at the shipped thresholds, the launch shapes, two contexts ---------------------------------------------------------
world = pytest.fixture(scope="module")(su.grid_world)

ASK_EVERY = 16384  # mapad_amd.hip: kTailAskEvery + 1 — a refused read asks again that many pops later
REASK_P0 = 256     # the pop budget of the re-ask cases: the first ask (MAPAD_TAIL_POPS_IDLE stays at 2^17, above it)
# 32-node base arenas: every read of consequence sits in a grown arena when it asks.  The ladder of classes above them ends at 16 384 nodes, so the reads of these
# cases need the last class (the reference's full limits, 336 MB an arena): 16 of those, and nobody leaves because a class is dry (MAPAD_TAIL_MIN_CLASS=10: such a read
# queues on the GPU, without popping) — every hand-over then happens at an ask point, which is what makes the arithmetic on gpu_pops exact.
REASK_ENV = {"MAPAD_TIER0_NODES": "32", "MAPAD_CLASS_COUNTS": "512,512,512,512,256,256,128,128,64,16", "MAPAD_TAIL_MIN_CLASS": "10"}


def reask_case(world):
    """-> (parameters, batch, the oracle's result).  sweep_util.grid_reads' recipe under CHEAPER_GAP, 4 000 reads instead of 300; of them every read the oracle needs more
    than P0 + 2 x 16 384 pops for (and fewer than 2^17: a quad makes 16 384 pops in 90 ms) and the first 200, most of them light."""
    rp, _ = su.grid_case("cheaper_gap")
    many = synth.reads(world.genome, 4000, 50, seed=31, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0), len_range=(35, 70), indel_frac=0.1)
    pops = world.oracle(("reask", "all"), rp, many).counters[:, 3]
    heavy = np.flatnonzero((pops > REASK_P0 + 2 * ASK_EVERY) & (pops < su.GRID_MAX_POPS))
    light = np.flatnonzero(pops[:200] < su.GRID_MAX_POPS)
    sel = np.unique(np.concatenate([heavy, light]))
    reads, qs = split_reads(*many)
    batch = su.pack([np.frombuffer(reads[i], np.uint8) for i in sel], [qs[i] for i in sel])
    return rp, batch, world.oracle(("reask", "chosen"), rp, batch)


@pytest.fixture(scope="module")
def reask(world):
    rp, batch, ores = reask_case(world)
    with pytest.MonkeyPatch.context() as mp:
        for k, v in REASK_ENV.items():
            mp.setenv(k, v)
        off, info_off = _map(world.pidx, mapad_amd.make_params(rp), *batch, tail_pops=0)  # the batch with the tail off: once, for the three cases
    assert info_off["reads"] == 0
    return rp, batch, ores, off


@pytest.mark.parametrize("case", ["budget_1", "budget_0", "budget_1_from_scratch"])
def test_refused_reads_ask_again(world, reask, case, monkeypatch):
    """A read past the budget that is refused goes on on the GPU and asks again every 16 384 pops.  Searches of tens of thousands of pops, a budget of 256 and a backlog
    limit of one: the reads ask in a crowd at 256 pops, one is taken at a time, the others go on, and the long ones are taken at their second, third, ... ask — out of a
    grown arena they have been in for tens of thousands of pops, with their state (budget_1) or without it (MAPAD_TAIL_CONTINUE=0).  With no room at all (budget_0)
    every one of them is refused at every ask — at least three times for the twenty-odd reads past 256 + 2 x 16 384 pops — and finishes on the GPU.
    Measured on an MI355X with 14 workers: 0.7 to 0.9 s a case; budget_1 handed 20 reads over, 14 of them with their state, after 27 asks beyond their first."""
    rp, batch, ores, off = reask
    pops = ores.counters[:, 3]
    assert int((pops > REASK_P0 + 2 * ASK_EVERY).sum()) >= 20 and int(pops.max()) < su.GRID_MAX_POPS
    past = int((pops > REASK_P0).sum())
    for k, v in REASK_ENV.items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("MAPAD_TAIL_POPS_IDLE", raising=False)
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", "0" if case == "budget_0" else "1")
    if case == "budget_1_from_scratch":
        monkeypatch.setenv("MAPAD_TAIL_CONTINUE", "0")
    res, info = _map(world.pidx, mapad_amd.make_params(rp), *batch, tail_pops=REASK_P0)
    print(case, info)
    assert_same_as_oracle(ores, res, batch[2])
    _same(res, off)
    assert (res.status & 16).sum() == 0
    assert info["reads_dry_class"] == 0 and info["reads_full_limit"] == 0 and info["reads_idle_tier"] == 0, info
    if case == "budget_0":
        assert info["reads"] == 0 and info["gpu_pops"] == 0 and info["host_pops"] == 0 and info["handed_over_with_state"] == 0, info
        return
    assert 0 < info["reads"] <= past, (info, past)  # (the first ask of the launch finds the ring empty and the pool idle)
    later = info["gpu_pops"] - REASK_P0 * info["reads"]
    assert later > 0 and later % ASK_EVERY == 0, info  # every hand-over happened at an ask point, and at least one at a later one than the first
    assert info["host_pops"] <= int(pops[pops > REASK_P0].sum())
    if case == "budget_1":
        assert 0 < info["continued"] <= info["handed_over_with_state"] <= info["reads"], info
    else:
        assert info["continued"] == 0 and info["handed_over_with_state"] == 0, info


class _Copies:
    """The oracle's result of ONE read as the result of a batch of k copies of it (what parity_util.assert_same_as_oracle reads of a result)."""

    def __init__(self, one, k):
        assert one.n == 1
        self.n, self._one = k, one
        h, o = int(one.hit_offsets[-1]), int(one.op_offsets[-1])
        self.hit_offsets = (np.arange(k + 1) * h).astype(one.hit_offsets.dtype)
        self.intervals, self.scores, self.ops = np.tile(one.intervals, (k, 1)), np.tile(one.scores, k), np.tile(one.ops, k)
        starts = (np.arange(k)[:, None] * o + np.asarray(one.op_offsets[:-1], np.int64)[None, :]).ravel()
        self.op_offsets = np.concatenate([starts, [k * o]]).astype(one.op_offsets.dtype)
        self.counters = np.tile(one.counters, (k, 1))

    def d_array(self, i):
        return self._one.d_array(0)


_TAIL_SWITCHES = ("MAPAD_TAIL_BACKLOG_BUDGET", "MAPAD_TAIL_BACKLOG_IDLE", "MAPAD_TAIL_BACKLOG", "MAPAD_TAIL_POPS_IDLE", "MAPAD_TAIL_MIN_CLASS", "MAPAD_TAIL_CONTINUE",
                  "MAPAD_TAIL_RING", "MAPAD_TAIL_THREADS", "MAPAD_TIER0_NODES", "MAPAD_CLASS_COUNTS")


def test_a_crowd_of_reads_asks_at_the_shipped_thresholds(world, monkeypatch):
    """No tail switch set, no set_tail_pops: the shipped gate.  k copies of sweep_util.explosive_case's read (2.9 M pops, 6.0 M edit-tree nodes) reach 2^17 pops in the
    same instant and ask for the host while a worker is idle — the crowd the CAS claim on the ring cursor was written for; k is more than the workers, so some are
    refused, go on, and leave at a later ask (or for a dry class, or at the full limit) as the workers drain.  Every copy's result is the oracle's of the one read.
    Measured on an MI355X with 14 workers, k = 20: 4.1 s; all twenty left while a worker was idle, with their state, the last six after 41 further asks between them."""
    for v in _TAIL_SWITCHES:
        monkeypatch.delenv(v, raising=False)
    rp, one = su.explosive_case(world)
    ores = world.oracle("explosive", rp, one)
    su.check_explosive_reach(ores)
    threads = int(mapad_amd.lib().mapad_tail_set_local_world(0))  # the pool's width under this environment
    k = threads + 6
    batch = su.pack([one[0]] * k, [one[1]] * k)
    ctx = mapad_amd.Context(world.pidx, mapad_amd.make_params(rp), 0)
    try:
        res = ctx.map_batch(*batch)
        info = ctx.tail_info()
    finally:
        ctx.close()
    print("crowd", k, info)
    assert_same_as_oracle(_Copies(ores, k), res, batch[2])
    assert (res.status & 16).sum() == 0
    assert info["threads"] == threads < k
    assert 1 <= info["reads"] <= k, info
    assert info["reads_idle_tier"] >= 1, info
    assert info["reads_idle_tier"] + info["reads_dry_class"] + info["reads_full_limit"] <= info["reads"], info
    assert info["continued"] <= info["handed_over_with_state"] <= info["reads"], info
    assert info["host_pops"] <= int(ores.counters[0, 3]) * info["reads"]
    if info["reads_idle_tier"] == info["reads"]:  # nobody left for a dry class, at the full limit or past the budget of 2^20 pops: every copy left at an ask point,
        later = info["gpu_pops"] - (1 << 17) * info["reads"]  # 2^17 pops and a multiple of 16 384 behind it
        # ... and not all at the first: the copies ask within microseconds of one another, the limit under the CAS is the number of workers, and a worker needs
        # a second for a copy — the copies beyond the workers are refused and go on
        assert later > 0 and later % ASK_EVERY == 0, info


def shapes_batch(world):
    return synth.reads(world.genome, 600, 50, seed=17, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0), len_range=(50, 100))


@pytest.mark.parametrize("lanes", ["2", "1"])
def test_pairs_and_single_lanes_hand_reads_over(world, lanes, monkeypatch):
    """The hand-over from the pair kernel (a heap top of its own size: never with state) and from single lanes (near data in global memory), out of grown arenas."""
    monkeypatch.setenv("MAPAD_LANES_PER_READ", lanes)
    monkeypatch.setenv("MAPAD_TIER0_NODES", "32")
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", GATES["unconditional"])
    rp = resolve_params(DAMAGE)
    batch = shapes_batch(world)
    ores = world.oracle(("shapes", "50-100"), rp, batch)
    pops, lens = ores.counters[:, 3], np.diff(batch[2].astype(np.int64))
    past = int((pops > 150).sum())
    assert lens.max() == 100 and pops[lens == lens.max()].min() > 150 and past >= 20  # the longest reads of the batch are among those handed over
    res, info = _map(world.pidx, mapad_amd.make_params(rp), *batch, tail_pops=150)
    assert_same_as_oracle(ores, res, batch[2])
    assert (res.status & 16).sum() == 0
    assert info["reads"] == past, (info, past)
    assert info["continued"] <= info["handed_over_with_state"] <= info["reads"], info
    print("lanes", lanes, info)
    assert info["gpu_pops"] >= 150 * _left_at_an_ask(info) and info["host_pops"] <= int(pops[pops > 150].sum())


# (lmax, lanes per read): the record's layout follows the batch's longest read (host_tail.hpp: tail_state_offset, tail_record_stride)
#   61: the qc block (2 x 61 bytes) is no multiple of 16;  256 | 257: quads with the near data in LDS | in global memory (hand_to_host reads it from there);
#   86: single lanes beyond their LDS limit;  299: pairs beyond theirs
_TAIL_LAYOUTS = [(61, "4"), (256, "4"), (257, "4"), (86, "1"), (299, "2")]


@pytest.mark.parametrize("lmax,lanes", _TAIL_LAYOUTS, ids=[f"{lmax}-lanes{lanes}" for lmax, lanes in _TAIL_LAYOUTS])
def test_hand_over_records_at_the_layout_thresholds(world, lmax, lanes, monkeypatch):
    monkeypatch.setenv("MAPAD_LANES_PER_READ", lanes)
    monkeypatch.setenv("MAPAD_TIER0_NODES", "32")
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", GATES["unconditional"])
    rp = su.b1_params("damage")
    batch = su.layout_batch(world.genome, lmax)
    ores = world.oracle(("b2", lmax), rp, batch)
    su.check_ladder_reach(ores, batch[2])
    pops, lens = ores.counters[:, 3], np.diff(batch[2].astype(np.int64))
    past = int((pops > 40).sum())
    assert lens.max() == lmax and pops[lens == lmax].min() > 40 and past >= 3  # the longest reads leave, with the whole extent of a record
    res, info = _map(world.pidx, mapad_amd.make_params(rp), *batch, tail_pops=40)
    assert_same_as_oracle(ores, res, batch[2])
    assert (res.status & 16).sum() == 0
    assert info["reads"] == past >= 3, (info, past)
    assert info["continued"] <= info["handed_over_with_state"] <= info["reads"], info
    print("lmax", lmax, info)
    assert info["gpu_pops"] >= 40 * _left_at_an_ask(info) and info["host_pops"] <= int(pops[pops > 40].sum())


def two_context_batches(world):
    return [synth.reads(world.genome, 1500, 50, seed=90 + i, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0)) for i in range(4)]


def test_two_contexts_with_tails_alive_at_once(world, gate):
    """The workers are one pool per process and the backlog word of every launch counts the tasks of all of them: two contexts on one device over one index, two
    batches submitted to each before anything is fetched — four launches whose tails are alive at once."""
    rp = resolve_params(DAMAGE)
    batches = two_context_batches(world)
    ctxs = []
    try:
        for _ in range(2):
            ctxs.append(mapad_amd.Context(world.pidx, mapad_amd.make_params(rp), 0))
            ctxs[-1].set_pipeline_depth(2)
            ctxs[-1].set_tail_pops(64)
        for j in range(2):
            for ci, ctx in enumerate(ctxs):
                ctx.submit_batch(*batches[2 * ci + j])
        got = {}
        for ci, ctx in enumerate(ctxs):
            for j in range(2):
                ctx.select_batch(1 - j)  # the older one first
                got[2 * ci + j] = (ctx.fetch(), ctx.tail_info())
    finally:
        for ctx in ctxs:
            ctx.close()
    for i, b in enumerate(batches):
        ores = world.oracle(("two_contexts", i), rp, b)
        pops = ores.counters[:, 3]
        res, info = got[i]
        assert_same_as_oracle(ores, res, b[2])
        assert (res.status & 16).sum() == 0
        if gate == "unconditional":
            assert info["reads"] == int((pops > 64).sum()) > 20, (i, info)
        else:  # only the first of the four launches finds the pool idle for certain
            assert _gated_counts(info, pops, 64, least=1 if i == 0 else 0) > 20
