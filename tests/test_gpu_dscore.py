"""The damage score on the GPU (run with -m gpu on an MI355X): what dscore_kernel writes while batches are converted to records — every read's score_q and
`scored`, the context's summary, and in mode 2 the reads the three analyses leave out — equals mapad_damage_score_host over the same fetched results and seeds
bit for bit, under every path a batch can take (both search steps, one quality level, duplicate collapsing, the host tail, batches in flight, the CLI), and
equals the scores decoded independently from the records / the BAM (tests/dscore_util.py)."""
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import build as mbuild
from mapad_amd import synth

import coverage_util as cu
import damage_util as du
import dscore_util as ds
import pileup_util as pu
from bam_util import read_bam
from kat_util import resolve_params
from parity_util import DAMAGE, DOUBLE_STRANDED, IGNORE_BQ

pytestmark = pytest.mark.gpu

DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 99
# TestDifferenceModel + TestBound: the alignment starts in the middle of the read, so the general-direction search step runs and the operations of a track are not
# in read order
TEST_MODEL = {"model": "test", "deam_score": -0.5, "mm_score": -1.0, "match_score": 0.0, "bound": "test", "threshold": -2.0, "repr_mm_bound": -1.0,
              "penalty_gap_open": -2.0, "penalty_gap_extend": -1.0, "gap_dist_ends": 5, "max_num_gaps_open": 1}
MODELS = {"ss": DAMAGE, "ds": DOUBLE_STRANDED, "test_model": TEST_MODEL, "ignore_bq": IGNORE_BQ}
GUARD = ["timeout", "-k", "10", "300"]  # every GPU child process under a time limit of its own
SPLIT = 250_000
LENGTHS = [SPLIT, 400_000 - SPLIT]


@pytest.fixture(scope="module")
def world():
    g = synth.genome(400_000, seed=77)
    g[300_000:300_400] = g[100_000:100_400]  # a repeat: reads from it have X0 > 1
    return g, mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])


def mixed_batch(g, n, seed):
    a = synth.reads(g, n, seed=seed, qual_range=(20, 40), damage=DMG, len_range=(20, 70), indel_frac=0.2)
    b = synth.reads(g[100_000:100_400], n // 10, 45, seed=seed + 1, exo_frac=0.0, damage=DMG)
    return pu.concat(a, b)


def seed_at(first_read):
    return int(mapad_amd.lib().mapad_records_seed_at(SEED, first_read))


def convert(ctx, res, batch, seed=SEED):
    """records on the device (which scores the batch) -> (records, text, score_q, scored)"""
    out = ctx.hits_to_records(res, *batch, seed=seed, as_arrays=True)
    assert len(out) == 4, "the records carry no scores"
    return out


def assert_same(got, want, what=""):
    """(score_q, scored, summary) of the device against the host path's: everything but kernel_ms"""
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0], want[0]), (what, np.flatnonzero(got[0] != want[0])[:10])
    ds.assert_summary(got[2], want[2], what)


@pytest.mark.parametrize("model", list(MODELS))
def test_device_scores_equal_the_host_path(world, model):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(MODELS[model]))
    batch = mixed_batch(g, 6000, seed=5)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_damage_score(1, 0.75)
        res = ctx.map_batch(*batch)
        _, _, score_q, scored = convert(ctx, res, batch)
        recs = ctx.hits_to_records(res, *batch, seed=SEED)  # the same batch again, as dicts: the same scores, nothing added
        got = ctx.damage_scores()
    finally:
        ctx.close()
    want = mb.damage_score_host(idx, params, res, *batch, seed=SEED, threshold=0.75)
    assert_same((score_q, scored, got), want, model)
    n = len(batch[2]) - 1
    assert got["batches"] == 1 and got["reads_seen"] == n and 0 < got["reads_scored"] < n and got["kernel_ms"] > 0.0 and got["threshold_q"] == 192
    assert 0 < got["reads_below"] < got["reads_scored"] and (score_q > 0).any()
    assert [r["damage_score"] for r in recs] == [float(q) / 256.0 if s else None for q, s in zip(score_q, scored)]
    assert all((r["damage_score"] is not None) == r["mapped"] for r in recs)
    if model in ("ss", "test_model"):  # and the scores decoded from the device's records in plain Python
        dq, dsc, dsum = ds.from_records(params, recs, batch, threshold_q=192)
        assert_same((score_q, scored, got), (dq, dsc, dsum), model + ": decoded from the records")
    if model == "ignore_bq":
        assert mapad_amd.damage_score_table(params, 50).shape == (50, 1, 4)


def test_smallest_batches_and_tracks_at_the_trip_boundaries(world):
    """one read; five reads (not a multiple of the block's four wavefronts); a batch with no mapped read; tracks of 63, 64, 65 and 129 operations (trips of 64 lanes)"""
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    rng = np.random.Generator(np.random.PCG64(3))
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def damaged(at, n):  # C -> T at the first and the last C: informative columns of both kinds in every trip
        r = g[at:at + n].copy()
        c = np.flatnonzero(r == ord("C"))
        r[c[[0, -1]]] = ord("T")
        return r

    long_reads = [damaged(20_000 + 500 * k, n) for k, n in enumerate((63, 64, 65, 129, 63, 64, 65, 129))] + [synth.revcomp(damaged(40_000, 129)), synth.revcomp(damaged(41_000, 64))]
    batches = {"one": pu.hand_made([damaged(10_000, 50)]), "five": pu.hand_made([damaged(11_000 + 100 * k, 40 + k) for k in range(5)]),
               "unmapped": pu.hand_made([acgt[rng.integers(0, 4, 50)] for _ in range(6)]), "trips": pu.hand_made(long_reads), "one_again": pu.hand_made([damaged(12_000, 33)])}
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_damage_score(2, 1.0)
        want_sum, first = None, 0
        for name, batch in batches.items():
            res = ctx.map_batch(*batch)
            recs, _, score_q, scored = convert(ctx, res, batch, seed=seed_at(first))
            wq, ws, want_sum = mb.damage_score_host(idx, params, res, *batch, seed=seed_at(first), threshold=1.0, into=want_sum)
            assert np.array_equal(score_q, wq) and np.array_equal(scored, ws), name
            k = len(batch[2]) - 1
            assert len(score_q) == k and (scored.all() if name != "unmapped" else not scored.any() and not score_q.any()), name
            if name == "trips":
                assert [int(r["cigar_len"]) for r in recs] == [3] * 3 + [4] + [3] * 3 + [4] + [4, 3]  # "63M" ... "129M": tracks of exactly that many operations
                assert (score_q > 0).all()
            first += k
        got = ctx.damage_scores()
    finally:
        ctx.close()
    ds.assert_summary(got, want_sum, "five small batches")
    assert got["batches"] == 5 and got["reads_seen"] == first and got["reads_scored"] == first - 6


def test_collapsing_and_the_host_tail_change_no_score(world, monkeypatch):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = du.with_duplicates(mixed_batch(g, 3000, seed=15), 2500, seed=3)
    want = mb.damage_score_host  # (called per result below: every result is its own fetch)
    got = {}
    for collapse in (True, False):
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_collapse_duplicates(collapse)
            ctx.set_damage_score(1)
            res = ctx.map_batch(*batch)
            if collapse:
                info = ctx.collapse_info()
                assert info[1] < info[0] == len(batch[2]) - 1
            _, _, score_q, scored = convert(ctx, res, batch)
            got[collapse] = (score_q, scored, ctx.damage_scores())
            assert_same(got[collapse], want(idx, params, res, *batch, seed=SEED), f"collapse={collapse}")
        finally:
            ctx.close()
    assert_same(got[True], got[False], "collapsed against not collapsed")
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", "4294967295")  # every read past the budget leaves for the host
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_tail_pops(48)
        ctx.set_damage_score(1)
        res = ctx.map_batch(*batch)
        assert ctx.tail_info()["reads"] > 100
        _, _, score_q, scored = convert(ctx, res, batch)
        tail = (score_q, scored, ctx.damage_scores())
    finally:
        ctx.close()
    assert_same(tail, want(idx, params, res, *batch, seed=SEED), "host tail")
    assert_same(tail, got[False], "host tail against the GPU alone")


def test_batches_in_flight_and_a_batch_converted_twice(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batches = [mixed_batch(g, 1500 + 300 * k, seed=40 + k) for k in range(5)]
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_pipeline_depth(3)
        ctx.set_damage_score(1, -0.5)
        want, flying, first = None, [], 0
        todo = list(batches)
        while todo or flying:
            while todo and len(flying) < 3:
                ctx.submit_batch(*todo[0])
                flying.append(todo.pop(0))
            ctx.select_batch(len(flying) - 1)  # the oldest
            b = flying.pop(0)
            res = ctx.fetch()
            _, _, score_q, scored = convert(ctx, res, b, seed=seed_at(first))
            wq, ws, want = mb.damage_score_host(idx, params, res, *b, seed=seed_at(first), threshold=-0.5, into=want)
            assert np.array_equal(score_q, wq) and np.array_equal(scored, ws)
            first += len(b[2]) - 1
        got = ctx.damage_scores()
        ds.assert_summary(got, want, "five batches, three in flight")
        assert got["batches"] == 5 and got["reads_seen"] == first
        # the last batch, still resident: converted again and through mapad_records_device it returns the same scores and adds nothing
        _, _, again_q, again_s = convert(ctx, res, b, seed=seed_at(first - (len(b[2]) - 1)))
        ctx.records_device(seed=SEED)
        assert np.array_equal(again_q, score_q) and np.array_equal(again_s, scored)
        ds.assert_summary(ctx.damage_scores(), got, "converted twice")
        assert ctx.damage_scores()["batches"] == 5
        ctx.reset_damage_scores()
        zero = ctx.damage_scores()
        assert zero["batches"] == 0 and zero["reads_seen"] == 0 and zero["score_sum"] == 0 and not zero["histogram"].any() and zero["kernel_ms"] == 0.0 and zero["threshold_q"] == -128
    finally:
        ctx.close()


def _analyses(ctx):
    return (ctx.pileup(3, 80), [ctx.pileup_counts(t, 0, n) for t, n in enumerate(LENGTHS)], ctx.coverage(), [ctx.coverage_depth(t, 0, n) for t, n in enumerate(LENGTHS)],
            ctx.damage_profile())


@pytest.mark.parametrize("dedup_mode", [0, 1, 2])
def test_mode_2_leaves_the_reads_below_the_threshold_out_of_the_three_analyses(world, dedup_mode):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = du.with_duplicates(mixed_batch(g, 3000, seed=55), 1500, seed=9)
    flt = (25, 2, 2)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        res = ctx.map_batch(*batch)
        hq, hs, _ = mb.damage_score_host(idx, params, res, *batch, seed=SEED)
        thr_q = int(np.sort(hq[hs == 1])[int(hs.sum()) // 2])  # a threshold that splits the batch, from the host's scores: both sides are non-empty
        below = (hs == 1) & (hq < thr_q)
        assert 0 < below.sum() < hs.sum()
        ctx.set_mark_duplicates(dedup_mode)
        ctx.set_pileup(1, *flt)
        ctx.set_coverage(1)
        ctx.set_damage_profile(1)
        ctx.set_damage_score(2, thr_q / 256.0)
        res = ctx.map_batch(*batch)
        recs, _, score_q, scored = convert(ctx, res, batch)
        p, pc, c, cd, d = _analyses(ctx)
        got = ctx.damage_scores()
    finally:
        ctx.close()
    assert np.array_equal(score_q, hq) and np.array_equal(scored, hs) and got["threshold_q"] == thr_q and got["reads_below"] == int(below.sum())
    dup = (recs["flags"] & 0x400) != 0
    assert dup.any() == (dedup_mode != 0)
    skip = (below | dup if dedup_mode == 2 else below).astype(np.uint8)  # mark-duplicates mode 1 marks and leaves nothing out
    if dedup_mode:
        assert (dup & ~below).any()
    pil = mb.PileupHost(idx, 1, *flt).add(params, res, *batch, seed=SEED, skip=skip)
    cov = mb.CoverageHost(idx, 1).add(params, res, seed=SEED, skip=skip)
    dmg = mapad_amd.damage_profile_host(idx, params, res, batch[0], batch[2], seed=SEED, mode=1, skip=skip)
    pu.assert_equal(p, pil.summary(3, 80), 3, 80, "pileup against the host path with skip")
    cu.assert_equal(c, cov.summary(), "coverage against the host path with skip")
    du.assert_equal(d, dmg, "damage profile against the host path with skip")
    for t, n in enumerate(LENGTHS):
        assert np.array_equal(pc[t], pil.counts(t, 0, n)) and np.array_equal(cd[t], cov.depth(t, 0, n))
    n = len(batch[2]) - 1
    assert p["reads_seen"] == c["reads_seen"] == d["reads_seen"] == n and c["reads"] == d["reads"] == int(hs.sum()) - int((skip.astype(bool) & (hs == 1)).sum())


def _record_texts(recs, text):
    """the CIGAR, MD and XA bytes of every record, in record order"""
    blob = text.tobytes()
    return [tuple(blob[int(r[k + "_off"]):int(r[k + "_off"]) + int(r[k + "_len"])] for k in ("cigar", "md", "xa")) for r in recs]


def _assert_same_records(a, b, same_pool):
    """every field of every record and the CIGAR, MD and XA bytes its offsets point to.  Pool offsets only on the host text path (same_pool): the device text
    pool is filled in arrival order."""
    assert len(a[0]) == len(b[0]) and _record_texts(a[0], a[1]) == _record_texts(b[0], b[1])
    for k in a[0].dtype.names:
        if k and not k.startswith("_") and (same_pool or not k.endswith("_off")):
            assert np.array_equal(a[0][k], b[0][k]), k
    if same_pool:
        assert a[1].tobytes() == b[1].tobytes()


def test_off_is_off_and_uploaded_hits_are_refused_only_while_on(world, monkeypatch):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 1500, seed=65)
    fresh, a, b = mapad_amd.Context(idx, params, 0), mapad_amd.Context(idx, params, 0), mapad_amd.Context(idx, params, 0)

    def both_paths(ctx, res):
        out = {"device": ctx.hits_to_records(res, *batch, seed=SEED, as_arrays=True)}
        with monkeypatch.context() as m:
            m.setenv("MAPAD_RECORDS_TEXT", "host")  # read at every records call
            out["host"] = ctx.hits_to_records(res, *batch, seed=SEED, as_arrays=True)
        return out

    try:
        want = both_paths(fresh, fresh.map_batch(*batch))
        assert all(len(v) == 2 for v in want.values())  # no scores beside the records
        never = fresh.damage_scores()
        assert never["batches"] == 0 and never["reads_seen"] == 0 and not never["histogram"].any()
        a.set_damage_score(2, 0.5)
        res_on = a.map_batch(*batch)
        on = both_paths(a, res_on)  # both records paths carry the same scores
        assert all(len(v) == 4 for v in on.values()) and np.array_equal(on["device"][2], on["host"][2]) and np.array_equal(on["device"][3], on["host"][3])
        assert_same((on["host"][2], on["host"][3], a.damage_scores()), mb.damage_score_host(idx, params, res_on, *batch, seed=SEED, threshold=0.5), "host text path")
        _assert_same_records(on["device"], want["device"], same_pool=False)  # the scores change no record
        _assert_same_records(on["host"], want["host"], same_pool=True)
        a.set_damage_score(0)
        off = both_paths(a, a.map_batch(*batch))
        assert all(len(v) == 2 for v in off.values())  # mapad_records_damage_scores returns NULL pointers
        _assert_same_records(off["device"], want["device"], same_pool=False)
        _assert_same_records(off["host"], want["host"], same_pool=True)
        assert a.damage_scores()["batches"] == 0 and "damage_score" not in a.hits_to_records(res_on, *batch, seed=SEED)[0]
        # another context's result: its hits are uploaded
        plain = fresh.hits_to_records(res_on, *batch, seed=SEED)
        assert b.hits_to_records(res_on, *batch, seed=SEED) == plain
        b.set_damage_score(1)
        with pytest.raises(mapad_amd.MapadError) as e:
            b.hits_to_records(res_on, *batch, seed=SEED)
        assert e.value.code == -9  # MAPAD_ERR_UNSUPPORTED
        assert b.damage_scores()["batches"] == 0
        b.set_damage_score(0)
        assert b.hits_to_records(res_on, *batch, seed=SEED) == plain
        for bad in ((3, 0.0), (-1, 0.0), (1, float("nan"))):
            with pytest.raises(mapad_amd.MapadError) as e:
                a.set_damage_score(*bad)
            assert e.value.code == -1
    finally:
        fresh.close()
        a.close()
        b.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def _read_hist(path):
    lines = open(path).read().splitlines()
    head = dict(kv.split("=") for kv in lines[0].split()[2:])
    assert lines[0].startswith("#mapad-amd-damage-score v1 ") and head["bins"] == "128"
    assert lines[1] == "#reads_seen\treads_scored\treads_below\tinformative_columns\tscore_sum_q\tbatches" and lines[3] == "#bin_start_bits\treads" and len(lines) == 4 + 128
    d = dict(zip(("reads_seen", "reads_scored", "reads_below", "informative_columns", "score_sum", "batches"), (int(x) for x in lines[2].split("\t"))))
    d["threshold_q"] = int(head["threshold_q"])
    rows = [ln.split("\t") for ln in lines[4:]]
    assert [float(r[0]) for r in rows] == [(k - 64) * 0.5 for k in range(128)]
    d["histogram"] = np.array([int(r[1]) for r in rows], np.uint64)
    return head, d


def test_cli_writes_the_scores_of_the_bam_it_writes(tmp_path):
    """DS:f of every mapped record of `mapad-amd map --damage_score` equals the score Python gets for the same reads (a context with the same parameters, and the
    scores decoded from the BAM's own CIGAR / MD / SEQ / QUAL); an input DS tag is dropped; the histogram file equals Context.damage_scores()."""
    mapad_amd.lib()
    cli = mbuild.build_cli()
    g = synth.genome(120_000, seed=17)
    fa, fq = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fastq")
    with open(fa, "w") as f:
        f.write(">chr1\n")
        s = g.tobytes().decode()
        for i in range(0, len(s), 60):
            f.write(s[i:i + 60] + "\n")
    batch = synth.reads(g, 2500, seed=23, qual_range=(20, 40), damage=DMG, len_range=(25, 80), indel_frac=0.2)
    seqs, quals, offsets = batch
    n = len(offsets) - 1
    with open(fq, "w") as f:
        for i in range(n):
            s, e = int(offsets[i]), int(offsets[i + 1])
            f.write(f"@r{i}\n{seqs[s:e].tobytes().decode()}\n+\n{''.join(chr(33 + q) for q in quals[s:e])}\n")
    subprocess.check_call(GUARD + [cli, "index", "-g", fa])
    base = GUARD + [cli, "map", "-r", fq, "-g", fa, "-l", "single_stranded", "-p", "0.03", "-f", "0.5", "-t", "0.5", "-d", "0.02", "-s", "1.0", "-i", "0.001", "--seed", "7",
                    "--batch_size", "1000"]
    params = mapad_amd.params_from_cli(library="single_stranded", five_prime_overhang=0.5, three_prime_overhang=0.5, ds_deamination_rate=0.02, ss_deamination_rate=1.0,
                                       poisson_prob=0.03, indel_rate=0.001)
    idx = mapad_amd.Index.build([("chr1", g)])
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_damage_score(2, 0.5)
        res = ctx.map_batch(*batch)
        _, _, score_q, scored = convert(ctx, res, batch, seed=7)
        want = ctx.damage_scores()
    finally:
        ctx.close()
    plain_bam = str(tmp_path / "plain.bam")
    subprocess.check_call(base + ["-o", plain_bam])
    assert all("DS" not in r["tags"] for r in read_bam(plain_bam)[2])
    for name, extra, thr_q, mode in (("score", ["--damage_score"], 0, "score"), ("filter", ["--damage_score_min", "0.5"], 128, "filter")):
        bam, tsv = str(tmp_path / f"{name}.bam"), str(tmp_path / f"{name}.tsv")
        pr = subprocess.run(base + ["-o", bam, "--damage_score_hist", tsv] + extra, check=True, stderr=subprocess.PIPE, text=True)
        assert "damage score (%s)" % mode in pr.stderr, pr.stderr
        recs = read_bam(bam)[2]
        assert len(recs) == n
        tables = {}
        for i, r in enumerate(recs):
            mapped = not r["flags"] & 0x4
            assert ("DS" in r["tags"]) == mapped == bool(scored[i]), i
            if mapped:
                assert r["tags"]["DS"][0] == "f" and np.float32(r["tags"]["DS"][1]) == np.float32(score_q[i]) / np.float32(256.0), i
                reverse = bool(r["flags"] & 0x10)
                read = r["seq"].translate(du._COMP)[::-1] if reverse else r["seq"]
                q = quals[int(offsets[i]):int(offsets[i + 1])]
                if len(read) not in tables:
                    tables[len(read)] = mapad_amd.damage_score_table(params, len(read))
                assert ds.score_record(tables[len(read)], read, q, True, reverse, r["cigar"], r["tags"]["MD"][1])[0] == int(score_q[i]), i
        head, d = _read_hist(tsv)
        assert head["mode"] == mode and d["batches"] == 3
        ds.assert_summary(d, dict(want, threshold_q=thr_q, batches=3, reads_below=int(((score_q < thr_q) & (scored == 1)).sum())), name)
    # an input DS tag is replaced by ours (the BAM of the run above as input: its DS tags, made wrong first, are dropped when ours is written)
    again = str(tmp_path / "again.bam")
    subprocess.check_call(GUARD + [cli, "map", "-r", str(tmp_path / "score.bam"), "-g", fa, "-l", "single_stranded", "-p", "0.03", "-f", "0.5", "-t", "0.5", "-d", "0.0", "-s", "0.0",
                                   "-i", "0.001", "--seed", "7", "--damage_score", "-o", again])
    recs = read_bam(again)[2]
    assert len(recs) == n and any(not r["flags"] & 0x4 for r in recs)
    for r in recs:  # -d 0 -s 0: every score is 0, and each record has exactly one DS tag
        if not r["flags"] & 0x4:
            assert r["tags"]["DS"] == ("f", 0.0) and r["tag_order"].count("DS") == 1
        else:
            assert "DS" not in r["tags"]
