"""PCR duplicates by alignment coordinates on the GPU (run with -m gpu on an MI355X): the flags the dedup_* kernels leave on a batch's records and the statistics
of the context's table equal mapad_dedup_host_* over the same fetched results and seeds, and equal a grouping built independently in numpy from the records
(tests/dedup_util.py) — under every path a batch can take (both search steps, both records paths, a table that grows, a wavefront on one slot, batches in
flight, duplicate collapsing, reads finished by the host tail, the CLI) —, and mode 2 leaves the flagged reads out of the damage profile, the coverage and the
pileup exactly as the host paths with skip= do."""
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import build as mbuild
from mapad_amd import synth

import coverage_util as cu
import damage_util as du
import dedup_util as dd
import pileup_util as pu
from bam_util import read_bam
from kat_util import resolve_params
from parity_util import DAMAGE

pytestmark = pytest.mark.gpu

DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 99
TEST_MODEL = {"model": "test", "deam_score": -0.5, "mm_score": -1.0, "match_score": 0.0, "bound": "test", "threshold": -2.0, "repr_mm_bound": -1.0,
              "penalty_gap_open": -2.0, "penalty_gap_extend": -1.0, "gap_dist_ends": 5, "max_num_gaps_open": 1}
MODELS = {"ss": DAMAGE, "test_model": TEST_MODEL}  # the backward-only and the general-direction search step (tests/test_gpu_pileup.py)
GUARD = ["timeout", "-k", "10", "300"]  # every GPU child process under a time limit of its own
SPLIT = 250_007
LENGTHS = [SPLIT, 400_000 - SPLIT]
_HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def world():
    g = synth.genome(400_000, seed=77)
    g[300_000:300_400] = g[100_000:100_400]  # a repeat: reads from it take the coordinate the seeded draw gives them
    return g, mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])


def library(g, n, copies, seed):
    """an amplified library: n drawn reads with indels, reads from the repeat, reads on the contigs' first and last bases, and `copies` of them drawn again, shuffled"""
    edges = pu.hand_made([g[0:40], g[SPLIT:SPLIT + 40], g[SPLIT - 40:SPLIT], g[400_000 - 40:400_000], synth.revcomp(g[SPLIT - 45:SPLIT])])
    drawn = pu.concat(synth.reads(g, n, seed=seed, qual_range=(20, 40), damage=DMG, len_range=(20, 150), indel_frac=0.3),
                      synth.reads(g[100_000:100_400], n // 10, 45, seed=seed + 1, exo_frac=0.0, damage=DMG), edges)
    return du.with_duplicates(drawn, copies, seed=seed + 2)


def cut(batch, k):
    """a batch in k consecutive pieces"""
    n = len(batch[2]) - 1
    ends = [n * (i + 1) // k for i in range(k)]
    return [du.take(batch, np.arange(a, b)) for a, b in zip([0] + ends[:-1], ends)]


def seed_at(first_read):
    return int(mapad_amd.lib().mapad_records_seed_at(SEED, first_read))


def run_batches(ctx, idx, params, batches, host=None):
    """every batch through ctx, converted in order -> (device flags, host flags, records, results), the flags and records of all batches one behind the other"""
    host = host if host is not None else mb.DedupHost()
    dev, hst, recs, results, first = [], [], [], [], 0
    for b in batches:
        res = ctx.map_batch(*b)
        r = ctx.hits_to_records(res, *b, seed=seed_at(first))
        dev.append(np.array([x["duplicate"] for x in r], np.uint8))
        assert all(bool(x["flags"] & 0x400) == x["duplicate"] for x in r)
        hst.append(host.add(idx, params, res, seed=seed_at(first)))
        recs += r
        results.append(res)
        first += len(b[2]) - 1
    return np.concatenate(dev), np.concatenate(hst), recs, results, host


def check_stats(got, host_summary, grouping_stats, what):
    dd.assert_stats(got, host_summary, what + ": device against the host path")
    dd.assert_stats(got, grouping_stats, what + ": device against the grouping of the records")
    h = np.asarray(got["histogram"], np.uint64).astype(np.int64)
    assert 0 < got["duplicates"] < got["reads_eligible"], what
    assert int(h.sum()) == got["fragments"], what
    if h[dd.BINS - 1] == 0:  # (the last bin is open-ended)
        assert int((h * np.arange(dd.BINS)).sum()) == got["reads_eligible"], what


@pytest.mark.parametrize("text", ["device", "host"])
@pytest.mark.parametrize("model", list(MODELS))
def test_device_flags_equal_the_host_path_and_the_grouping(world, model, text, monkeypatch):
    if text == "host":
        monkeypatch.setenv("MAPAD_RECORDS_TEXT", "host")
    g, idx = world
    params = mapad_amd.make_params(resolve_params(MODELS[model]))
    batches = cut(library(g, 3000, 1500, seed=5), 2)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_mark_duplicates(1)
        dev, hst, recs, _, host = run_batches(ctx, idx, params, batches)
        got = ctx.duplicates()
    finally:
        ctx.close()
    want, stats = dd.from_records(recs)
    what = f"{model}, records text on the {text}"
    assert np.array_equal(dev, hst), (what, np.flatnonzero(dev != hst)[:10])
    assert np.array_equal(dev, want), (what, np.flatnonzero(dev != want)[:10])
    check_stats(got, host.summary(), stats, what)
    h = np.asarray(got["histogram"], np.int64)
    assert int((h * np.arange(dd.BINS)).sum()) == got["reads_eligible"] and h[dd.BINS - 1] == 0 and h[0] == 0
    n = sum(len(b[2]) - 1 for b in batches)
    assert got["batches"] == 2 and got["reads_seen"] == n and got["reads_eligible"] < n and got["mark_ms"] > 0.0 and got["summary_ms"] > 0.0
    assert got["slots"] >= 2 * got["fragments"] and got["slots"] == host.summary()["slots"] and got["grows"] == host.summary()["grows"]
    # the library is what it is meant to be: both strands, gaps, reads from the repeat among the flagged
    flagged = [r for r, f in zip(recs, dev) if f]
    assert {r["reverse"] for r in flagged} == {False, True} and any(r["xt"] == "R" for r in flagged) and all(r["mapped"] for r in flagged)
    if model == "ss":
        assert any("I" in r["cigar"] for r in flagged) and any("D" in r["cigar"] for r in flagged)


def test_a_table_that_grows_gives_the_same_flags(world, monkeypatch):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    whole = library(g, 3800, 800, seed=15)  # about 5 000 reads, in three batches of growing size: each of them outgrows the table the one before left
    n = len(whole[2]) - 1
    batches = [du.take(whole, np.arange(a, b)) for a, b in ((0, n * 16 // 100), (n * 16 // 100, n * 44 // 100), (n * 44 // 100, n))]
    out = {}
    for slots in ("64", "65536"):
        monkeypatch.setenv("MAPAD_DEDUP_SLOTS", slots)  # read when the mode is set / the host accumulator is made
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_mark_duplicates(1)
            dev, hst, recs, _, host = run_batches(ctx, idx, params, batches)
            out[slots] = (dev, ctx.duplicates(), recs)
            assert np.array_equal(dev, hst)
            assert out[slots][1]["grows"] == host.summary()["grows"] and out[slots][1]["slots"] == host.summary()["slots"]
        finally:
            ctx.close()
    small, large = out["64"], out["65536"]
    assert small[1]["grows"] >= 3 and large[1]["grows"] == 0 and large[1]["slots"] == 65536 and small[1]["slots"] >= 2 * small[1]["fragments"]
    assert np.array_equal(small[0], large[0]) and np.array_equal(small[0], dd.from_records(small[2])[0])
    dd.assert_stats(small[1], large[1], "a table that grew against one that did not")
    assert 0 < small[1]["duplicates"] < small[1]["reads_eligible"]


def test_a_wavefront_on_one_slot(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    one = pu.hand_made([g[123_456:123_506]] * 64)
    batch = pu.concat(one, library(g, 1000, 300, seed=25), one)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_mark_duplicates(1)
        dev, hst, recs, _, host = run_batches(ctx, idx, params, [batch])
        got = ctx.duplicates()
    finally:
        ctx.close()
    assert all(r["mapped"] and r["pos"] == 123_456 and not r["reverse"] for r in recs[:64])
    assert dev[0] == 0 and dev[1:64].all() and dev[-64:].all()  # exactly the first read is the original
    assert np.array_equal(dev, hst) and np.array_equal(dev, dd.from_records(recs)[0])
    assert got["histogram"][128] >= 1
    dd.assert_stats(got, host.summary(), "a wavefront on one slot")


def test_batches_in_flight_and_a_batch_converted_twice(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batches = cut(library(g, 3000, 1500, seed=35), 4)  # groups straddle the cuts
    empty = (np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    rng = np.random.Generator(np.random.PCG64(1))
    junk = pu.hand_made([np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 60)] for _ in range(50)])
    ctx = mapad_amd.Context(idx, params, 0)
    host = mb.DedupHost()
    try:
        ctx.set_pipeline_depth(2)
        ctx.set_mark_duplicates(1)
        dev, hst, recs, first = [], [], [], 0
        flying, todo = [], list(batches)
        while todo or flying:
            while todo and len(flying) < 2:
                ctx.submit_batch(*todo[0])
                flying.append(todo.pop(0))
            ctx.select_batch(len(flying) - 1)  # the oldest: batches are converted in order
            b = flying.pop(0)
            res = ctx.fetch()
            r = ctx.hits_to_records(res, *b, seed=seed_at(first))
            again = ctx.hits_to_records(res, *b, seed=seed_at(first))  # converted twice: the same flags, no counter moves
            assert again == r
            dev.append(np.array([x["duplicate"] for x in r], np.uint8))
            hst.append(host.add(idx, params, res, seed=seed_at(first)))
            recs += r
            first += len(b[2]) - 1
        dev, hst = np.concatenate(dev), np.concatenate(hst)
        got = ctx.duplicates()
        want, stats = dd.from_records(recs)
        assert np.array_equal(dev, hst) and np.array_equal(dev, want)
        check_stats(got, host.summary(), stats, "four batches at depth 2, each converted twice")
        assert got["batches"] == 4 and got["reads_seen"] == first
        per_batch = sum(int(dd.from_records(recs[a:b])[0].sum()) for a, b in zip(np.cumsum([0] + [len(x[2]) - 1 for x in batches])[:-1], np.cumsum([len(x[2]) - 1 for x in batches])))
        assert got["duplicates"] > per_batch  # reads flagged for a read of an earlier batch
        # a batch with no reads and a batch with no mapped read: a batch more each, and nothing else
        for k, b in enumerate((empty, junk)):
            res = ctx.map_batch(*b)
            r = ctx.hits_to_records(res, *b, seed=SEED)
            assert not any(x["mapped"] or x["duplicate"] for x in r)
            now = ctx.duplicates()
            assert now["batches"] == 5 + k and now["reads_seen"] == first + (50 if k else 0)
            assert all(now[f] == got[f] for f in ("reads_eligible", "duplicates", "fragments")) and np.array_equal(now["histogram"], got["histogram"])
        # reset: nothing has been seen; the batch still resident is marked anew, from ordinal 0
        ctx.duplicates_reset()
        zero = ctx.duplicates()
        assert zero["batches"] == 0 and zero["reads_seen"] == 0 and zero["fragments"] == 0 and not zero["histogram"].any() and zero["slots"] == got["slots"]
    finally:
        ctx.close()


def test_collapsing_and_the_host_tail_change_no_flag(world, monkeypatch):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = library(g, 2000, 1500, seed=45)
    flags = {}
    for what in ("plain", "collapse", "tail"):
        if what == "tail":
            monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", "4294967295")  # every read past the budget leaves for the host
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_collapse_duplicates(what == "collapse")
            if what == "tail":
                ctx.set_tail_pops(48)
            ctx.set_mark_duplicates(1)
            res = ctx.map_batch(*batch)
            if what == "collapse":
                info = ctx.collapse_info()
                assert info[1] < info[0] == len(batch[2]) - 1
            if what == "tail":
                assert ctx.tail_info()["reads"] > 100
            recs = ctx.hits_to_records(res, *batch, seed=SEED)
            flags[what] = np.array([x["duplicate"] for x in recs], np.uint8)
            assert np.array_equal(flags[what], mb.DedupHost().add(idx, params, res, seed=SEED)) and np.array_equal(flags[what], dd.from_records(recs)[0]), what
            assert 0 < ctx.duplicates()["duplicates"] == int(flags[what].sum())
        finally:
            ctx.close()
    assert np.array_equal(flags["plain"], flags["collapse"]) and np.array_equal(flags["plain"], flags["tail"])


def _analyses(ctx):
    return (ctx.pileup(3, 80), [ctx.pileup_counts(t, 0, n) for t, n in enumerate(LENGTHS)], ctx.coverage(), [ctx.coverage_depth(t, 0, n) for t, n in enumerate(LENGTHS)],
            ctx.damage_profile())


def test_mode_2_leaves_the_duplicates_out_of_the_three_analyses(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batches = cut(library(g, 3000, 2000, seed=55), 2)
    flt = (25, 2, 2)
    got = {}
    for mode in (0, 1, 2):
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_mark_duplicates(mode)
            ctx.set_pileup(1, *flt)
            ctx.set_coverage(1)
            ctx.set_damage_profile(1)
            dev, hst, recs, results, _ = run_batches(ctx, idx, params, batches)
            got[mode] = (dev, recs, results, _analyses(ctx))
        finally:
            ctx.close()
    assert not got[0][0].any() and np.array_equal(got[1][0], got[2][0]) and got[2][0].any()
    # mode 1 leaves all three as they are with the mode off
    for mode in (1,):
        p, pc, c, cd, d = got[mode][3]
        p0, pc0, c0, cd0, d0 = got[0][3]
        pu.assert_equal(p, p0, 3, 80, "pileup, mode 1 against off")
        cu.assert_equal(c, c0, "coverage, mode 1 against off")
        du.assert_equal(d, d0, "damage, mode 1 against off")
        assert all(np.array_equal(x, y) for x, y in zip(pc, pc0)) and all(np.array_equal(x, y) for x, y in zip(cd, cd0))
    # mode 2: the host _skip paths, and the numpy tables of the records with the duplicates masked
    flags, recs, results, (p, pc, c, cd, d) = got[2]
    pil, cov, dmg, first = mb.PileupHost(idx, 1, *flt), mb.CoverageHost(idx, 1), None, 0
    for b, res in zip(batches, results):
        k = len(b[2]) - 1
        skip = flags[first:first + k]
        pil.add(params, res, *b, seed=seed_at(first), skip=skip)
        cov.add(params, res, seed=seed_at(first), skip=skip)
        dmg = mapad_amd.damage_profile_host(idx, params, res, b[0], b[2], seed=seed_at(first), mode=1, into=dmg, skip=skip)
        first += k
    pu.assert_equal(p, pil.summary(3, 80), 3, 80, "pileup, mode 2 against the host path with skip")
    cu.assert_equal(c, cov.summary(), "coverage, mode 2 against the host path with skip")
    du.assert_equal(d, dmg, "damage, mode 2 against the host path with skip")
    for t, n in enumerate(LENGTHS):
        assert np.array_equal(pc[t], pil.counts(t, 0, n)) and np.array_equal(cd[t], cov.depth(t, 0, n))
    whole = pu.concat(*batches)
    kept = dd.masked(recs, flags)
    pu.assert_equal(p, pu.from_records(LENGTHS, kept, whole, 1, *flt), 3, 80, "pileup, mode 2 against numpy", counts_of=lambda t, s, k: pc[t][s:s + k])
    cu.assert_equal(c, cu.from_records(LENGTHS, kept, 1), "coverage, mode 2 against numpy", depth_of=lambda t, s, k: cd[t][s:s + k])
    du.assert_equal(d, du.from_records(kept, whole[0], whole[2], 1), "damage, mode 2 against numpy")
    assert p["reads"] < got[0][3][0]["reads"] and p["reads_seen"] == got[0][3][0]["reads_seen"] and c["reads"] == p["reads"] == d["reads"]


def _record_texts(recs, text):
    """the CIGAR, MD and XA bytes of every record, in record order"""
    blob = text.tobytes()
    return [tuple(blob[int(r[k + "_off"]):int(r[k + "_off"]) + int(r[k + "_len"])] for k in ("cigar", "md", "xa")) for r in recs]


def _assert_only_the_flag_differs(recs_on, recs_off, same_pool):
    """every field of every record and every byte of its text, 0x400 apart.  The text kernel's wavefronts claim their room in the text pool in the order in which
    they get there, so where a record's text lies in the pool is no property of the record: on the device text path the offsets are followed and the strings
    compared; the host text path writes the pool in read order, and there (same_pool) the offsets and the pool itself are compared as well."""
    assert (recs_on[0]["flags"] & 0x400).any() and not (recs_off[0]["flags"] & 0x400).any()
    assert len(recs_on[0]) == len(recs_off[0]) and _record_texts(*recs_on) == _record_texts(*recs_off)
    for k in recs_on[0].dtype.names:  # (field by field: the structure's padding bytes are not part of a record)
        if k and not k.startswith("_") and (same_pool or not k.endswith("_off")):
            on = recs_on[0][k] & ~np.uint16(0x400) if k == "flags" else recs_on[0][k]
            assert np.array_equal(on, recs_off[0][k]), k
    if same_pool:
        assert recs_on[1].tobytes() == recs_off[1].tobytes()


def test_off_is_off_and_uploaded_hits_are_refused_only_while_on(world, monkeypatch):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = library(g, 1500, 800, seed=65)
    a, b = mapad_amd.Context(idx, params, 0), mapad_amd.Context(idx, params, 0)

    def both_paths(ctx, res):
        out = {"device": ctx.hits_to_records(res, *batch, seed=SEED, as_arrays=True)}
        with monkeypatch.context() as m:
            m.setenv("MAPAD_RECORDS_TEXT", "host")  # read at every records call
            out["host"] = ctx.hits_to_records(res, *batch, seed=SEED, as_arrays=True)
        return out

    try:
        res_off = a.map_batch(*batch)
        recs_off = both_paths(a, res_off)
        off = a.duplicates()
        assert off["batches"] == 0 and off["reads_seen"] == 0 and off["slots"] == 0 and not off["histogram"].any()
        a.set_mark_duplicates(1)
        res = a.map_batch(*batch)
        recs_on = both_paths(a, res)  # (the second conversion of the batch returns the flags of the first)
        _assert_only_the_flag_differs(recs_on["device"], recs_off["device"], same_pool=False)
        _assert_only_the_flag_differs(recs_on["host"], recs_off["host"], same_pool=True)
        assert np.array_equal(recs_on["device"][0]["flags"], recs_on["host"][0]["flags"])
        in_flags = np.full(len(batch[2]) - 1, 0x400 | 0x200, np.uint16)
        assert ((a.hits_to_records(res, *batch, in_flags=in_flags, seed=SEED, as_arrays=True)[0]["flags"] & 0x600) == 0x600).all()  # on top of in_flags
        want = a.hits_to_records(res, *batch, seed=SEED)
        plain = [dict(r, duplicate=False, flags=r["flags"] & ~0x400) for r in want]
        assert b.hits_to_records(res, *batch, seed=SEED) == plain  # another context's result: uploaded hits, the mode off there
        b.set_mark_duplicates(1)
        with pytest.raises(mapad_amd.MapadError) as e:
            b.hits_to_records(res, *batch, seed=SEED)
        assert e.value.code == -9  # MAPAD_ERR_UNSUPPORTED
        assert b.duplicates()["batches"] == 0
        b.set_mark_duplicates(0)
        assert b.hits_to_records(res, *batch, seed=SEED) == plain
        for bad in (3, -1):
            with pytest.raises(mapad_amd.MapadError) as e:
                a.set_mark_duplicates(bad)
            assert e.value.code == -1
        a.set_mark_duplicates(0)  # frees the table
        assert a.duplicates()["slots"] == 0
    finally:
        a.close()
        b.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def _read_report(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("#mapad-amd-duplicates v1 ") and lines[1] == "#reads_seen\treads_eligible\tduplicates\tfragments\tslots\tgrows\tbatches" and lines[3] == "#members\tfragments"
    head = dict(kv.split("=") for kv in lines[0].split()[2:])
    scalars = dict(zip(lines[1][1:].split("\t"), (int(x) for x in lines[2].split("\t"))))
    hist = np.zeros(dd.BINS, np.uint64)
    rows = [tuple(int(x) for x in ln.split("\t")) for ln in lines[4:]]
    assert [k for k, _ in rows] == list(range(1, dd.BINS))
    for k, v in rows:
        hist[k] = v
    scalars["histogram"] = hist
    return head, scalars


def test_cli_marks_the_duplicates_of_the_bam_it_writes(tmp_path):
    mapad_amd.lib()
    cli = mbuild.build_cli()
    g = synth.genome(120_000, seed=17)
    g[90_000:90_300] = g[30_000:30_300]
    split = 70_003
    lengths = [split, 120_000 - split]
    fa, fq = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fastq")
    with open(fa, "w") as f:
        for name, s in (("chr1", g[:split].tobytes().decode()), ("chr2", g[split:].tobytes().decode())):
            f.write(f">{name}\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    u = synth.reads(g, 2500, seed=23, qual_range=(20, 40), damage=DMG, len_range=(25, 110), indel_frac=0.3)
    rep = synth.reads(g[30_000:30_300], 150, 40, seed=24, qual_range=(20, 40), exo_frac=0.0)
    edges = pu.hand_made([g[0:40], g[split:split + 40], g[split - 40:split], g[120_000 - 40:120_000]], qual=31)
    seqs, quals, offsets = du.with_duplicates(pu.concat(u, rep, edges), 1346, seed=13)
    n_reads = len(offsets) - 1
    with open(fq, "w") as f:
        for i in range(n_reads):
            a, b = int(offsets[i]), int(offsets[i + 1])
            f.write(f"@r{i}\n{seqs[a:b].tobytes().decode()}\n+\n{''.join(chr(33 + q) for q in quals[a:b])}\n")
    subprocess.check_call(GUARD + [cli, "index", "-g", fa])
    base = GUARD + [cli, "map", "-r", fq, "-g", fa, "-l", "single_stranded", "-p", "0.03", "-f", "0.5", "-t", "0.5", "-d", "0.02", "-s", "1.0", "-i", "0.001", "--seed", "7"]

    def run(name, extra):
        bam = str(tmp_path / f"{name}.bam")
        pr = subprocess.run(base + ["-o", bam] + extra, check=True, stderr=subprocess.PIPE, text=True)
        return read_bam(bam)[2], pr.stderr

    plain, _ = run("plain", [])
    assert len(plain) == n_reads == 4000 and not any(r["flags"] & 0x400 for r in plain)
    report = str(tmp_path / "dup.tsv")
    marked, err = run("marked", ["--mark_duplicates", "--duplicates", report])
    assert "duplicates (marked)" in err, err
    want, stats = dd.from_bam(marked)
    assert np.array_equal(np.array([bool(r["flags"] & 0x400) for r in marked], np.uint8), want)
    head, scalars = _read_report(report)
    assert head == {"mode": "mark", "bins": "256"} and scalars["batches"] >= 1 and scalars["slots"] >= 2 * scalars["fragments"]
    dd.assert_stats(scalars, stats, "the report against the grouping over the BAM")
    assert 0 < scalars["duplicates"] < scalars["reads_eligible"] < n_reads == scalars["reads_seen"]
    # the flag is all that differs from a run without the option
    strip = lambda recs: [(r["name"], r["flags"] & ~0x400, r["tid"], r["pos"], r["mapq"], r["cigar"], r["seq"], r["qual"]) for r in recs]  # noqa: E731
    assert strip(marked) == strip(plain)
    # the flagged read names do not depend on --batch_size
    small, _ = run("small", ["--mark_duplicates", "--batch_size", "500"])
    names = lambda recs: [r["name"] for r in recs if r["flags"] & 0x400]  # noqa: E731
    assert names(small) == names(marked) and len(names(marked)) == scalars["duplicates"]
    # --exclude_duplicates: the pileup of the unflagged records
    tsv = str(tmp_path / "pileup.tsv")
    excluded, err = run("excluded", ["--exclude_duplicates", "--pileup", tsv])
    assert "duplicates (excluded)" in err and names(excluded) == names(marked)
    kept = [dict(r, flags=r["flags"] | 0x4) if r["flags"] & 0x400 else r for r in excluded]
    table = pu.from_bam(lengths, kept, 1)
    lines = open(tsv).read().splitlines()
    got = dict(zip(lines[1][1:].split("\t"), (int(x) for x in lines[2].split("\t"))))
    assert all(got[k] == table[k] for k in pu.SCALARS) and got["reads"] == scalars["fragments"]
    for t, ln in enumerate(lines[4:]):
        f = ln.split("\t")
        w = pu.contig_stats(table["counts"][t], 1, 0)
        assert [int(x) for x in f[1:]] == [w["length"], w["sites_covered"], w["sites_deep"], w["sites_called"]] + w["called"] + w["base_sum"] + [w["max_depth"]]
    # more than one device: refused with a message, whichever option asks
    for opt in ("--mark_duplicates", "--exclude_duplicates"):
        cmd = GUARD + [cli, "--devices", "0,0"] + base[len(GUARD) + 1:] + ["-o", str(tmp_path / "two.bam"), opt]
        pr = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        assert pr.returncode not in (0, 124, 137) and "one device only" in pr.stderr, pr.stderr
    pr = subprocess.run(base + ["-o", str(tmp_path / "bad.bam"), "--duplicates", report], stderr=subprocess.PIPE, text=True)
    assert pr.returncode not in (0, 124, 137) and "--duplicates FILE needs" in pr.stderr
