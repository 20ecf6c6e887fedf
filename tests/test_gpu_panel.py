"""The SNP panel on the GPU (run with -m gpu on an MI355X): what panel_kernel accumulates in a context while batches are converted to records, and what
panel_call_kernel makes of it, equals mapad_snp_panel_host_* over the same fetched results, reads and seeds — counters, strand-split counts, row statistics and
calls, bit for bit — under every path a batch can take (both search steps, duplicate collapsing, reads finished by the host tail, batches in flight, two contexts
merged, reads left out by the duplicate marks and the damage score, rescaled qualities, the CLI), and equals the table built independently in numpy from the
records / the BAM (tests/panel_util.py)."""
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import build as mbuild
from mapad_amd import synth

import damage_util as du
import panel_util as pn
import pileup_util as pu
from bam_util import read_bam
from kat_util import resolve_params
from parity_util import DAMAGE

pytestmark = pytest.mark.gpu

SEED = 99
# TestDifferenceModel + TestBound: the alignment starts in the middle of the read, so the general-direction search step runs and the operations of a track are not
# in read order.  (Its threshold of -2 admits no gap, so deletions are asserted for "ss" only.)
TEST_MODEL = {"model": "test", "deam_score": -0.5, "mm_score": -1.0, "match_score": 0.0, "bound": "test", "threshold": -2.0, "repr_mm_bound": -1.0,
              "penalty_gap_open": -2.0, "penalty_gap_extend": -1.0, "gap_dist_ends": 5, "max_num_gaps_open": 1}
MODELS = {"ss": DAMAGE, "test_model": TEST_MODEL}
GUARD = ["timeout", "-k", "10", "600"]  # every GPU child process under a time limit of its own
LENGTHS = pn.LENGTHS
FILTERS = [(0, 0, 0), (30, 3, 2)]  # (min_bq, mask5, mask3)
RULE = dict(call=0, min_depth=1, transitions=2, seed=31)


@pytest.fixture(scope="module")
def world():
    g = pn.world_genome()
    return g, mapad_amd.Index.build([("c1", g[:pn.SPLIT]), ("c2", g[pn.SPLIT:])]), pn.panel(g)


def host_of(idx, params, p, res, batch, mode, flt=(0, 0, 0), seed=SEED, into=None, skip=None):
    return (into if into is not None else mb.SnpPanelHost(idx, mode, *pn.args(p), *flt)).add(params, res, *batch, seed=seed, skip=skip)


def assert_device_equals_host(ctx, acc, n_rows, what="", rules=(RULE,)):
    assert np.array_equal(ctx.snp_panel_counts(0, n_rows), acc.counts(0, n_rows)), (what, "counts")
    for rule in rules:
        got, want = ctx.snp_panel(rule), acc.summary(rule)
        for k in pn.SCALARS + pn.WORDS + ("mode", "min_base_quality", "mask5", "mask3", "n_rows", "n_slots", "rule"):
            assert got[k] == want[k], (what, rule, k, got[k], want[k])
        assert np.array_equal(ctx.snp_panel_calls(0, n_rows, rule), acc.calls(0, n_rows, rule)), (what, rule, "calls")
    return got


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("model", list(MODELS))
def test_device_panel_equals_the_host_path_and_the_records(world, model, mode):
    g, idx, p = world
    params = mapad_amd.make_params(resolve_params(MODELS[model]))
    batch = pn.mixed_batch(g, 5000, seed=5)
    n, n_rows = len(batch[2]) - 1, len(p["tid"])
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_snp_panel(mode, *pn.args(p), *FILTERS[0])
        res = ctx.map_batch(*batch)
        for flt in FILTERS:
            ctx.set_snp_panel(mode, *pn.args(p), *flt)  # (a panel set again starts an empty table: the batch, still resident, counts into it)
            recs = ctx.hits_to_records(res, *batch, seed=SEED)
            what = f"{model}, mode {mode}, filters {flt}"
            got = assert_device_equals_host(ctx, host_of(idx, params, p, res, batch, mode, flt), n_rows, what, rules=pn.RULES)
            want = pn.from_records(LENGTHS, recs, batch, p, mode, *flt)
            pn.assert_equal(ctx.snp_panel, ctx.snp_panel_counts, ctx.snp_panel_calls, want, LENGTHS, p, what + ": numpy table from the device's records")
            assert got["batches"] == 1 and got["reads_seen"] == n and 0 < got["reads_on_panel"] < got["reads"] < n and got["accumulate_ms"] > 0.0 and got["summary_ms"] > 0.0
            assert got["columns_not_acgt"] > 0 and got["rows_called"] > 0 and got["rows_unplaced"] == 5 and got["rows_bad_alleles"] == 4
            if flt != (0, 0, 0):
                assert got["columns_masked"] > 0 and got["columns_low_quality"] > 0
            else:
                assert got["columns_masked"] == 0 and got["columns_low_quality"] == 0
                ends = {(int(t), int(x)): i for i, (t, x) in enumerate(zip(p["tid"], p["pos0"])) if (int(t), int(x)) in ((0, 0), (0, pn.SPLIT - 1), (1, 0), (1, LENGTHS[1] - 1))}
                assert len(ends) == 4 and all(ctx.snp_panel_counts(i, 1).sum() >= 1 for i in ends.values())  # reads on a contig's first and last base hit their slots
    finally:
        ctx.close()
    # the batch exercises the hard shapes
    counted = [r for r in recs if r["mapped"] and (mode == 1 or r["xt"] == "U")]
    site = [np.zeros(k, bool) for k in LENGTHS]
    ok = pn.placed(LENGTHS, p)
    for t, x in zip(p["tid"][ok], p["pos0"][ok]):
        site[int(t)][int(x)] = True
    span = lambda r: sum(int(k) for k, op in pu._CIGAR.findall(r["cigar"]) if op != "I")  # noqa: E731
    slots = [int(site[r["tid"]][r["pos"]:r["pos"] + span(r)].sum()) for r in counted]
    assert max(slots) > 64 and min(slots) == 0
    if model == "ss":
        assert got["columns_deleted"] > 0
        assert {r["reverse"] for r in counted if "D" in r["cigar"] and r["tid"] == 0 and pn.DENSE_START <= r["pos"] < pn.DENSE_START + pn.DENSE_LEN} == {False, True}
    if mode == 2:
        assert got["reads"] < sum(1 for r in recs if r["mapped"])


def test_duplicates_count_like_every_other_read(world):
    g, idx, p = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = du.with_duplicates(pn.mixed_batch(g, 3000, seed=15), 2500, seed=3)
    n_rows = len(p["tid"])
    got = {}
    for collapse in (True, False):
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_collapse_duplicates(collapse)
            ctx.set_snp_panel(1, *pn.args(p), 30, 3, 2)
            res = ctx.map_batch(*batch)
            if collapse:
                info = ctx.collapse_info()
                assert info[1] < info[0] == len(batch[2]) - 1
            ctx.hits_to_records(res, *batch, seed=SEED)
            assert_device_equals_host(ctx, host_of(idx, params, p, res, batch, 1, (30, 3, 2)), n_rows, f"collapse={collapse}")
            got[collapse] = (ctx.snp_panel_counts(0, n_rows), ctx.snp_panel_calls(0, n_rows, RULE))
        finally:
            ctx.close()
    assert np.array_equal(got[True][0], got[False][0]) and np.array_equal(got[True][1], got[False][1])


def test_reads_finished_by_the_host_tail_count(world, monkeypatch):
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", "4294967295")  # every read past the budget leaves for the host
    g, idx, p = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = pn.mixed_batch(g, 3000, seed=25)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_tail_pops(48)
        ctx.set_snp_panel(2, *pn.args(p), 25, 2, 2)
        res = ctx.map_batch(*batch)
        assert ctx.tail_info()["reads"] > 100
        ctx.hits_to_records(res, *batch, seed=SEED)
        assert_device_equals_host(ctx, host_of(idx, params, p, res, batch, 2, (25, 2, 2)), len(p["tid"]))
    finally:
        ctx.close()


def _run_pipeline(ctx, idx, params, p, batches, mode, flt, acc=None, first_read=0):
    """the batches through ctx at pipeline depth 2, each converted once; -> (the host accumulator over the same results, reads so far)"""
    flying, todo = [], list(batches)
    while todo or flying:
        while todo and len(flying) < 2:
            ctx.submit_batch(*todo[0])
            flying.append(todo.pop(0))
        ctx.select_batch(len(flying) - 1)  # the oldest
        b = flying.pop(0)
        res = ctx.fetch()
        seed = int(mapad_amd.lib().mapad_records_seed_at(SEED, first_read))
        ctx.hits_to_records(res, *b, seed=seed)
        acc = host_of(idx, params, p, res, b, mode, flt, seed=seed, into=acc)
        first_read += len(b[2]) - 1
    return acc, first_read


def _error_of(call):
    try:
        call()
    except mapad_amd.MapadError as e:
        return e.code
    return None


def test_batches_in_flight_accumulate_and_two_contexts_merge(world):
    g, idx, p = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    empty = (np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    batches = [pn.mixed_batch(g, 1500 + 300 * k, seed=40 + k) for k in range(3)]
    flt, n_rows = (30, 3, 2), len(p["tid"])
    one, a, b = (mapad_amd.Context(idx, params, 0) for _ in range(3))
    try:
        for c in (one, a, b):
            c.set_pipeline_depth(2)
            c.set_snp_panel(1, *pn.args(p), *flt)
        acc, n = _run_pipeline(one, idx, params, p, batches, 1, flt)
        got = assert_device_equals_host(one, acc, n_rows, "three batches at depth 2", rules=pn.RULES)
        assert got["batches"] == 3 and got["reads_seen"] == n
        res = one.map_batch(*empty)  # an empty batch launches nothing and counts as none, on the device and on the host
        assert len(one.hits_to_records(res, *empty, seed=SEED)) == 0
        after = assert_device_equals_host(one, host_of(idx, params, p, res, empty, 1, flt, into=acc), n_rows, "an empty batch behind them")
        assert after["batches"] == 3 and after["reads_seen"] == n
        # two contexts that took one half of the batches each, merged: the context that took all
        _, n_a = _run_pipeline(a, idx, params, p, batches[:2], 1, flt)
        _run_pipeline(b, idx, params, p, batches[2:], 1, flt, first_read=n_a)
        half = a.snp_panel(RULE)
        assert half["batches"] == 2 and half["reads"] < got["reads"]
        a.snp_panel_merge(b)
        merged = assert_device_equals_host(a, acc, n_rows, "merged", rules=pn.RULES)
        assert merged["batches"] == 3 and b.snp_panel(RULE)["batches"] == 1  # the source keeps its own
        # another filter, another mode, another panel (one allele, one position, one row less), off: not the same table
        other = {k: v.copy() for k, v in p.items()}
        other["alt"][0] = ord("A") if other["alt"][0] != ord("A") else ord("C")
        moved = {k: v.copy() for k, v in p.items()}
        moved["pos0"][1] += 1
        short = {k: v[:-1] for k, v in p.items()}
        for setting in ((1, p, (30, 3, 1)), (1, p, (29, 3, 2)), (2, p, flt), (1, other, flt), (1, moved, flt), (1, short, flt), (0, p, flt)):
            b.set_snp_panel(setting[0], *pn.args(setting[1]), *setting[2])
            assert _error_of(lambda: a.snp_panel_merge(b)) == -1  # MAPAD_ERR_INVALID
        assert _error_of(lambda: a.snp_panel_merge(a)) == -1
        assert_device_equals_host(a, acc, n_rows, "after the refused merges")
    finally:
        for c in (one, a, b):
            c.close()


def test_a_batch_counts_once_reset_zeroes_and_off_is_off(world):
    g, idx, p = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = pn.mixed_batch(g, 3000, seed=55)
    n_rows = len(p["tid"])
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        res_off = ctx.map_batch(*batch)  # mode 0, the default
        recs_off = ctx.hits_to_records(res_off, *batch, seed=SEED)
        off = ctx.snp_panel()
        assert off["mode"] == 0 and off["n_rows"] == 0 and off["batches"] == 0 and all(off[k] == 0 for k in pn.SCALARS + pn.WORDS)
        assert len(ctx.snp_panel_counts(0, 0)) == 0 and _error_of(lambda: ctx.snp_panel_counts(0, 1)) == -1
        ctx.set_snp_panel(1, *pn.args(p))
        res = ctx.map_batch(*batch)
        recs = ctx.hits_to_records(res, *batch, seed=SEED)
        # off and on: the same results and the same records, byte for byte
        assert recs == recs_off and np.array_equal(res.hit_begin, res_off.hit_begin) and np.array_equal(res.ops, res_off.ops)
        acc = host_of(idx, params, p, res, batch, 1)
        once = assert_device_equals_host(ctx, acc, n_rows, "once")
        ctx.hits_to_records(res, *batch, seed=SEED)  # the same result again, then the same batch through mapad_records_device
        ctx.records_device(seed=SEED)
        again = assert_device_equals_host(ctx, acc, n_rows, "converted three times")
        assert again["batches"] == once["batches"] == 1
        ctx.snp_panel_reset()
        zero = ctx.snp_panel(RULE)
        assert zero["batches"] == 0 and zero["reads_seen"] == 0 and zero["rows_called"] == 0 and zero["rows"] == n_rows and zero["mode"] == 1
        assert not ctx.snp_panel_counts(0, n_rows).any() and bytes(ctx.snp_panel_calls(0, 3, RULE)) == b"999"
        ctx.hits_to_records(res, *batch, seed=SEED)  # nothing has been counted: the batch, still resident, counts into the fresh table
        assert_device_equals_host(ctx, acc, n_rows, "after the reset")
        for bad in (lambda: ctx.snp_panel(dict(min_depth=0)), lambda: ctx.snp_panel(dict(call=2)), lambda: ctx.snp_panel_calls(0, 4, dict(transitions=3)),
                    lambda: ctx.snp_panel_counts(n_rows - 3, 4), lambda: ctx.snp_panel_calls(n_rows, 1), lambda: ctx.set_snp_panel(3, *pn.args(p)),
                    lambda: ctx.set_snp_panel(1, *pn.args(p), 256), lambda: ctx.set_snp_panel(1, *pn.args(p), 0, 65536),
                    lambda: ctx.set_snp_panel(1, np.zeros(0, np.int32), np.zeros(0, np.uint64), b"", b"")):
            assert _error_of(bad) == -1  # MAPAD_ERR_INVALID
        assert_device_equals_host(ctx, acc, n_rows, "after the refused calls")
        ctx.set_snp_panel(0)
        res = ctx.map_batch(*batch)
        ctx.hits_to_records(res, *batch, seed=SEED)
        assert ctx.snp_panel()["mode"] == 0 and ctx.snp_panel()["batches"] == 0
    finally:
        ctx.close()


def test_uploaded_hits_are_refused_only_while_the_panel_is_on(world):
    g, idx, p = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = pn.mixed_batch(g, 1000, seed=65)
    a, b = mapad_amd.Context(idx, params, 0), mapad_amd.Context(idx, params, 0)
    try:
        res = a.map_batch(*batch)
        want = a.hits_to_records(res, *batch, seed=SEED)
        assert b.hits_to_records(res, *batch, seed=SEED) == want  # another context's result: its hits are uploaded, its reads are not on the device
        b.set_snp_panel(1, *pn.args(p))
        assert _error_of(lambda: b.hits_to_records(res, *batch, seed=SEED)) == -9  # MAPAD_ERR_UNSUPPORTED
        assert b.snp_panel()["batches"] == 0
        b.set_snp_panel(0)
        assert b.hits_to_records(res, *batch, seed=SEED) == want
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("dedup_mode", [0, 2])
def test_reads_left_out_by_the_duplicate_marks_and_the_damage_score_are_left_out(world, dedup_mode):
    g, idx, p = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = du.with_duplicates(pn.mixed_batch(g, 3000, seed=56), 1500, seed=9)
    flt, n_rows = (25, 2, 2), len(p["tid"])
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        res = ctx.map_batch(*batch)
        hq, hs, _ = mb.damage_score_host(idx, params, res, *batch, seed=SEED)
        thr_q = int(np.sort(hq[hs == 1])[int(hs.sum()) // 2])  # a threshold that splits the batch, from the host's scores
        below = (hs == 1) & (hq < thr_q)
        ctx.set_mark_duplicates(dedup_mode)
        ctx.set_snp_panel(1, *pn.args(p), *flt)
        ctx.set_damage_score(2, thr_q / 256.0)
        res = ctx.map_batch(*batch)
        dup = np.array([r["duplicate"] for r in ctx.hits_to_records(res, *batch, seed=SEED)], bool)
        assert dup.any() == (dedup_mode != 0) and 0 < below.sum() < hs.sum()
        skip = (below | dup).astype(np.uint8)
        got = assert_device_equals_host(ctx, host_of(idx, params, p, res, batch, 1, flt, skip=skip), n_rows, f"mark-duplicates mode {dedup_mode}, damage-score mode 2")
        everyone = host_of(idx, params, p, res, batch, 1, flt).summary(RULE)
        assert got["reads_seen"] == everyone["reads_seen"] and got["reads"] == everyone["reads"] - int((skip.astype(bool) & (hs == 1)).sum())
        if dedup_mode == 2:  # the duplicate marks alone
            ctx.set_damage_score(0)
            ctx.snp_panel_reset()
            ctx.hits_to_records(res, *batch, seed=SEED)
            assert_device_equals_host(ctx, host_of(idx, params, p, res, batch, 1, flt, skip=dup.astype(np.uint8)), n_rows, "mark-duplicates mode 2 alone")
    finally:
        ctx.close()


def test_rescale_mode_2_feeds_the_panel_filter_and_mode_1_does_not(world):
    g, idx, p = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = pn.mixed_batch(g, 3000, seed=57)
    flt, n_rows = (25, 0, 0), len(p["tid"])
    seqs, quals, offsets = batch
    got = {}
    for mode in (1, 2):
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_snp_panel(1, *pn.args(p), *flt)
            ctx.set_quality_rescale(mode)
            res = ctx.map_batch(*batch)
            ctx.hits_to_records(res, *batch, seed=SEED)
            host_q, _ = mb.quality_rescale_host(idx, params, res, *batch, seed=SEED)
            q = quals if mode == 1 else host_q  # mode 1: the input qualities; mode 2: the host-rescaled ones
            got[mode] = assert_device_equals_host(ctx, host_of(idx, params, p, res, (seqs, q, offsets), 1, flt), n_rows, f"rescale mode {mode}")
        finally:
            ctx.close()
    assert got[2]["columns_low_quality"] > got[1]["columns_low_quality"] and got[2]["columns_counted"] < got[1]["columns_counted"]


def _readouts(ctx):
    """every existing stage's read-out, without the times"""
    out = {"dup": ctx.duplicates(), "ds": ctx.damage_scores(), "rs": ctx.quality_rescale(), "dmg": ctx.damage_profile(), "cov": ctx.coverage(), "pil": ctx.pileup(3, 80),
           "al": ctx.allele_summary(2, 1.0), "gt": ctx.genotype_summary(2, 1.0, 2.0)}

    def strip(v):
        if isinstance(v, dict):
            return {k: strip(x) for k, x in v.items() if not k.endswith("_ms")}
        if isinstance(v, (list, tuple)):
            return [strip(x) for x in v]
        return v.tolist() if isinstance(v, np.ndarray) else v
    out = strip(out)
    out["pil_counts"] = [ctx.pileup_counts(t, 0, n) for t, n in enumerate(LENGTHS)]
    out["cov_depth"] = [ctx.coverage_depth(t, 0, n) for t, n in enumerate(LENGTHS)]
    out["al_cells"] = [ctx.allele_cells(t, 0, n) for t, n in enumerate(LENGTHS)]
    out["gt_cells"] = [ctx.genotype_cells(t, 0, n) for t, n in enumerate(LENGTHS)]
    return out


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_the_panel_beside_the_pileup_and_every_other_stage(world):
    g, idx, p = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = du.with_duplicates(pn.mixed_batch(g, 3000, seed=58), 1000, seed=4)
    flt, n_rows = (30, 3, 2), len(p["tid"])
    got = {}
    for panel_on in (False, True):
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_mark_duplicates(1)
            ctx.set_damage_score(1)
            ctx.set_quality_rescale(1)
            ctx.set_damage_profile(1)
            ctx.set_coverage(1)
            ctx.set_pileup(1, *flt)
            ctx.set_allele_likelihoods(1, *flt)
            ctx.set_genotype_likelihoods(True)
            if panel_on:
                ctx.set_snp_panel(1, *pn.args(p), *flt)
            res = ctx.map_batch(*batch)
            recs = ctx.hits_to_records(res, *batch, seed=SEED)
            got[panel_on] = (_readouts(ctx), recs)
            if panel_on:
                counts = ctx.snp_panel_counts(0, n_rows)
                ok = pn.placed(LENGTHS, p)
                pile = got[True][0]["pil_counts"]
                at = [pile[int(t)][int(x)] for t, x in zip(p["tid"][ok], p["pos0"][ok])]
                assert np.array_equal(counts[ok].sum(axis=1), np.array(at)) and not counts[~ok].any() and counts.any()
                assert_device_equals_host(ctx, host_of(idx, params, p, res, batch, 1, flt), n_rows, "beside the eight other stages")
        finally:
            ctx.close()
    assert _same(got[False][0], got[True][0]) and got[False][1] == got[True][1]


@pytest.mark.parametrize("size", ["one", "64", "65", "a whole contig"])
def test_panel_sizes(world, size):
    g, idx, _ = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    if size == "a whole contig":  # one slot per position of c2: every read of c2 walks, every column of it is counted
        n = LENGTHS[1]
        p = {"tid": np.ones(n, np.int32), "pos0": np.arange(n, dtype=np.uint64), "ref": g[pn.SPLIT:].copy(), "alt": pn._next(g[pn.SPLIT:], 2)}
    else:
        n = int(size) if size != "one" else 1
        x = np.sort(np.random.default_rng(n).choice(2_000, n, replace=False)).astype(np.uint64) + 16_000  # among the hand-made reads of the dense stretch
        p = {"tid": np.zeros(n, np.int32), "pos0": x, "ref": g[x.astype(np.int64)].copy(), "alt": pn._next(g[x.astype(np.int64)], 1)}
    batch = pu.concat(pn.mixed_batch(g, 1500, seed=70), synth.reads(g[15_500:18_500], 1500, seed=71, qual_range=(20, 40), damage=pn.DMG, len_range=(20, 150), indel_frac=0.3))
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_snp_panel(1, *pn.args(p), 25, 2, 1)
        res = ctx.map_batch(*batch)
        recs = ctx.hits_to_records(res, *batch, seed=SEED)
        got = assert_device_equals_host(ctx, host_of(idx, params, p, res, batch, 1, (25, 2, 1)), n, size, rules=pn.RULES)
        want = pn.from_records(LENGTHS, recs, batch, p, 1, 25, 2, 1)
        pn.assert_equal(ctx.snp_panel, ctx.snp_panel_counts, ctx.snp_panel_calls, want, LENGTHS, p, size) if n >= 200 else None
        assert np.array_equal(ctx.snp_panel_counts(0, n).astype(np.int64), want["counts"]) and got["n_slots"] == n and got["columns_counted"] > 0
        if size == "a whole contig":
            pile = mb.PileupHost(idx, 1, 25, 2, 1).add(params, res, *batch, seed=SEED)
            assert np.array_equal(ctx.snp_panel_counts(0, n).sum(axis=1), pile.counts(1, 0, n))
    finally:
        ctx.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_panel_of_the_bam_it_wrote(tmp_path):
    """`mapad-amd map --snp_panel`: the BAM holds the same records as a run without; .geno, the counts TSV and the report equal the numpy table of that BAM and
    what SnpPanelHost gives for the same reads through the binding; .snp is the input, .ind names the sample; chromosome names fall back; --batch_size and
    --collapse_duplicates change nothing; --exclude_duplicates and single_strand do what they say"""
    from test_gpu_pileup import _decoded
    mapad_amd.lib()
    cli = mbuild.build_cli()
    g = synth.genome(120_000, seed=17)
    g[90_000:90_300] = g[30_000:30_300]
    split = 70_003
    lengths = [split, 120_000 - split]
    fa, fq, snp = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fastq"), str(tmp_path / "panel.snp")
    with open(fa, "w") as f:
        for name, s in (("chr1", g[:split].tobytes().decode()), ("X", g[split:].tobytes().decode())):
            f.write(f">{name}\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    u = synth.reads(g, 3000, seed=23, qual_range=(20, 40), damage=pn.DMG, len_range=(25, 110), indel_frac=0.3)
    rep = synth.reads(g[30_000:30_300], 200, 40, seed=24, qual_range=(20, 40), exo_frac=0.0)
    edges = pu.hand_made([g[0:40], g[split:split + 40], g[split - 40:split], g[120_000 - 40:120_000]], qual=31)
    batch = du.with_duplicates(pu.concat(u, rep, edges), 1296, seed=13)
    seqs, quals, offsets = batch
    n_reads = len(offsets) - 1
    with open(fq, "w") as f:
        for i in range(n_reads):
            s, e = int(offsets[i]), int(offsets[i + 1])
            f.write(f"@r{i}\n{seqs[s:e].tobytes().decode()}\n+\n{''.join(chr(33 + q) for q in quals[s:e])}\n")
    # the panel: every 37th position (alternating transversions and transitions), the contigs' ends, chromosome "1" for chr1 and "23" for X, rows that name no contig
    xs = sorted(set(range(0, 120_000, 37)) | {0, split - 1, split, 120_000 - 1})
    tid = np.array([0 if x < split else 1 for x in xs] + [-1, -1], np.int32)
    pos0 = np.array([x - (split if x >= split else 0) for x in xs] + [5, 0], np.uint64)
    ref = np.concatenate([g[xs], np.frombuffer(b"AN", np.uint8)])
    alt = np.concatenate([pn._next(g[xs], 1 + (np.arange(len(xs)) & 1)), np.frombuffer(b"CA", np.uint8)])
    p = {"tid": tid, "pos0": pos0, "ref": ref, "alt": alt}
    lines = [f"rs{i}\t{'1' if t == 0 else '23'}\t{i * 1e-6:.6f}\t{int(x) + 1}\t{chr(r)}\t{chr(a)}" for i, (t, x, r, a) in enumerate(zip(tid[:-2], pos0[:-2], ref[:-2], alt[:-2]))]
    lines += ["nowhere\t7\t0.0\t6\tA\tC", "zero\t1\t0.0\t0\tN\tA"]
    open(snp, "w").write("".join(ln + "\n" for ln in lines))
    n_rows = len(lines)
    subprocess.check_call(GUARD + [cli, "index", "-g", fa])
    base = GUARD + [cli, "map", "-r", fq, "-g", fa, "-l", "single_stranded", "-p", "0.03", "-f", "0.5", "-t", "0.5", "-d", "0.02", "-s", "1.0", "-i", "0.001", "--seed", "7"]
    subprocess.check_call(base + ["--batch_size", "1000", "-o", str(tmp_path / "plain.bam")])
    plain = _decoded(str(tmp_path / "plain.bam"))
    assert len(plain[2]) == n_reads
    idx = mapad_amd.Index.open(fa)

    def run(name, extra, batch_size="1000"):
        out = {k: str(tmp_path / f"{name}.{k}") for k in ("bam", "geno", "snp", "ind", "tsv", "report")}
        cmd = base + ["--batch_size", batch_size, "-o", out["bam"], "--snp_panel", snp, "--panel_geno", out["geno"], "--panel_snp", out["snp"], "--panel_ind", out["ind"],
                      "--panel_counts", out["tsv"], "--panel_report", out["report"]] + extra
        pr = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True)
        assert "snp panel (" in pr.stderr and "rows called" in pr.stderr, pr.stderr
        return out

    def check(name, extra, mode, flt, rule, same_bam=True, dup_out=False, **kw):
        out = run(name, extra, **kw)
        if same_bam:
            assert _decoded(out["bam"]) == plain, name
        bam = read_bam(out["bam"])[2]
        if dup_out:
            assert any(r["flags"] & 0x400 for r in bam)
            bam = [r for r in bam if not r["flags"] & 0x400]
        want = pn.from_bam(lengths, bam, p, mode, *flt)
        calls, words, _ = pn.calls(lengths, p, want["counts"], **rule)
        geno = open(out["geno"]).read()
        assert geno == "".join(chr(c) + "\n" for c in calls), name
        assert open(out["snp"]).read() == open(snp).read()
        tsv = open(out["tsv"]).read().splitlines()
        call_name, tr_name = ("random", "majority")[rule["call"]], ("keep", "missing", "single_strand")[rule["transitions"]]
        assert tsv[0] == (f"#mapad-amd-snp-panel v1 mode={'unique' if mode == 2 else 'all'} min_bq={flt[0]} mask5={flt[1]} mask3={flt[2]} call={call_name} "
                          f"min_depth={rule['min_depth']} transitions={tr_name} seed={rule['seed']}")
        assert tsv[1] == "#id\tchrom\tpos\tref\talt\tfwd_A\tfwd_C\tfwd_G\tfwd_T\trev_A\trev_C\trev_G\trev_T\tcall" and len(tsv) == 2 + n_rows
        for i, ln in enumerate(tsv[2:]):
            f = ln.split("\t")
            assert f[:5] == lines[i].split("\t")[:2] + lines[i].split("\t")[3:] and [int(v) for v in f[5:13]] == want["counts"][i].reshape(8).tolist() and f[13] == chr(calls[i]), (name, i)
        report = dict(ln.split("\t") for ln in open(out["report"]).read().splitlines())
        assert (report["mode"], report["call"], report["transitions"], report["min_depth"], report["seed"]) == ("unique" if mode == 2 else "all", call_name, tr_name,
                                                                                                                 str(rule["min_depth"]), str(rule["seed"]))
        assert (report["min_bq"], report["mask5"], report["mask3"]) == tuple(str(v) for v in flt) and int(report["n_rows"]) == n_rows and int(report["batches"]) >= 1
        for k in pn.SCALARS:
            if not (dup_out and k == "reads_seen"):
                assert int(report[k]) == want[k], (name, k)
        for k in pn.WORDS:
            assert int(report[k]) == words[k], (name, k)
        assert words["rows_unplaced"] == 2 and words["rows_called"] > 100 and want["reads_on_panel"] > 0
        return out, want, calls

    rule0 = dict(call=0, min_depth=1, transitions=0, seed=0)
    first, want, calls = check("default", [], 1, (0, 0, 0), rule0)
    assert open(first["ind"]).read() == "sample\tU\tUnknown\n"
    assert want["columns_masked"] == 0 and want["columns_low_quality"] == 0
    # the binding's host path over the same reads and seed: the same counts and calls
    params = mapad_amd.params_from_cli(library="single_stranded", five_prime_overhang=0.5, three_prime_overhang=0.5, ds_deamination_rate=0.02, ss_deamination_rate=1.0,
                                       poisson_prob=0.03, indel_rate=0.001)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        res = ctx.map_batch(*batch)
        acc = mb.SnpPanelHost(idx, 1, *pn.args(p)).add(params, res, *batch, seed=7)
        assert np.array_equal(acc.counts(0, n_rows).astype(np.int64), want["counts"]) and np.array_equal(acc.calls(0, n_rows, rule0), calls)
    finally:
        ctx.close()
    # another chunking, duplicate collapsing, coalesced launches: byte for byte the same files
    other = run("one_chunk_collapsed", ["--collapse_duplicates", "--coalesce", "2"], batch_size="100000")
    for k in ("geno", "tsv", "snp", "ind"):
        assert open(other[k]).read() == open(first[k]).read(), k
    named, flt_want, _ = check("filtered_majority_single_strand", ["--panel_min_bq", "30", "--panel_mask5", "3", "--panel_mask3", "2", "--panel_call", "majority", "--panel_min_depth", "2",
                                                                   "--panel_transitions", "single_strand", "--panel_seed", "18446744073709551615", "--panel_sample", "Ind1",
                                                                   "--panel_population", "Pop"], 1, (30, 3, 2), dict(call=1, min_depth=2, transitions=2, seed=2**64 - 1))
    assert open(named["ind"]).read() == "Ind1\tU\tPop\n" and flt_want["columns_masked"] > 0 and flt_want["columns_low_quality"] > 0
    _, unique, _ = check("unique_missing", ["--panel_unique", "--panel_transitions", "missing", "--panel_seed", "5"], 2, (0, 0, 0), dict(call=0, min_depth=1, transitions=1, seed=5))
    assert unique["reads"] < want["reads"]
    _, nodup, _ = check("exclude_duplicates", ["--exclude_duplicates"], 1, (0, 0, 0), rule0, same_bam=False, dup_out=True)
    assert nodup["reads"] < want["reads"]
    # beside the pileup in one run: each file as in its own run
    both = run("beside_the_pileup", ["--pileup", str(tmp_path / "both_pileup.tsv"), "--coverage", str(tmp_path / "both_cov.tsv")])
    assert open(both["geno"]).read() == open(first["geno"]).read() and open(both["tsv"]).read() == open(first["tsv"]).read() and _decoded(both["bam"]) == plain
    for bad in (["--panel_geno", str(tmp_path / "x.geno")], ["--snp_panel", snp], ["--snp_panel", snp, "--panel_geno", str(tmp_path / "x.geno"), "--panel_min_depth", "0"],
                ["--snp_panel", snp, "--panel_geno", str(tmp_path / "x.geno"), "--panel_call", "best"], ["--snp_panel", snp, "--panel_geno", str(tmp_path / "x.geno"), "--panel_sample", "S"]):
        assert subprocess.run(base + ["-o", str(tmp_path / "bad.bam")] + bad, stderr=subprocess.DEVNULL).returncode != 0  # flags without their panel; a depth of 0; ...
