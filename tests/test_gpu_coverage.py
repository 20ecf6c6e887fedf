"""Depth of coverage on the GPU (run with -m gpu on an MI355X): what coverage_kernel accumulates in a context while batches are converted to records, and what
the finishing pass makes of it, equals mapad_coverage_host_* over the same fetched results and seeds — summary and per-base depth — under every path a batch can
take (both search kernels, duplicate collapsing, reads finished by the host tail, batches in flight, two contexts merged, the CLI), and equals the table built
independently in numpy from the records / the BAM (tests/coverage_util.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import build as mbuild
from mapad_amd import synth

import coverage_util as cu
import damage_util as du
from bam_util import read_bam
from kat_util import resolve_params
from parity_util import DAMAGE

pytestmark = pytest.mark.gpu

DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 99
# TestDifferenceModel + TestBound: the alignment starts in the middle of the read, so the general-direction search step runs and the operations of a track are not
# in read order
TEST_MODEL = {"model": "test", "deam_score": -0.5, "mm_score": -1.0, "match_score": 0.0, "bound": "test", "threshold": -2.0, "repr_mm_bound": -1.0,
              "penalty_gap_open": -2.0, "penalty_gap_extend": -1.0, "gap_dist_ends": 5, "max_num_gaps_open": 1}
MODELS = {"ss": DAMAGE, "test_model": TEST_MODEL}
GUARD = ["timeout", "-k", "10", "600"]  # every GPU child process under a time limit of its own
SPLIT = 250_007  # where the two contigs meet: no multiple of a segment size (64, 16384)
LENGTHS = [SPLIT, 400_000 - SPLIT]


@pytest.fixture(scope="module")
def world():
    g = synth.genome(400_000, seed=77)
    g[300_000:300_400] = g[100_000:100_400]  # a repeat: reads from it have X0 > 1 (mode 2 leaves them out)
    return g, mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])


def mixed_batch(g, n, seed):
    """reads of 20..150 bases with indels (tracks longer than a wavefront, deletions on both strands), reads from the repeat, and reads on the contigs' first and
    last bases and across a segment boundary"""
    edges = cu.hand_made([g[0:40], g[SPLIT:SPLIT + 40], g[SPLIT - 40:SPLIT], g[400_000 - 40:400_000], synth.revcomp(g[SPLIT - 45:SPLIT]), g[16_360:16_410], g[SPLIT + 40:SPLIT + 90]])
    return cu.concat(synth.reads(g, n, seed=seed, qual_range=(20, 40), damage=DMG, len_range=(20, 150), indel_frac=0.3),
                     synth.reads(g[100_000:100_400], n // 10, 45, seed=seed + 1, exo_frac=0.0, damage=DMG), edges)


def host_of(idx, params, res, mode, seed=SEED, into=None):
    return (into if into is not None else mb.CoverageHost(idx, mode)).add(params, res, seed=seed)


def assert_device_equals_host(ctx, acc, what=""):
    got = ctx.coverage()
    cu.assert_equal(got, acc.summary(), what)
    for t, n in enumerate(LENGTHS):
        assert np.array_equal(ctx.coverage_depth(t, 0, n), acc.depth(t, 0, n)), (what, "depth of contig", t)
    return got


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("model", list(MODELS))
def test_device_coverage_equals_the_host_path_and_the_records(world, model, mode, monkeypatch):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(MODELS[model]))
    batch = mixed_batch(g, 5000, seed=5)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_coverage(mode)
        res = ctx.map_batch(*batch)
        recs = ctx.hits_to_records(res, *batch, seed=SEED)
        acc = host_of(idx, params, res, mode)
        want = cu.from_records(LENGTHS, recs, mode)
        for segment in ("64", None):  # 64: thousands of segments, the contigs' ends inside segments; then the default
            if segment is None:
                monkeypatch.delenv("MAPAD_COVERAGE_SEGMENT", raising=False)
            else:
                monkeypatch.setenv("MAPAD_COVERAGE_SEGMENT", segment)
            what = f"{model}, mode {mode}, segment {segment}"
            got = assert_device_equals_host(ctx, acc, what)
            cu.assert_equal(got, want, what + ": numpy table from the device's records", depth_of=ctx.coverage_depth)
            for t, d in enumerate(want["depth"]):  # windows that start in the middle of a contig, at non-zero depth
                for start in (int(np.argmax(d)), LENGTHS[t] - 30):
                    n_win = min(5000, LENGTHS[t] - start)
                    assert d[start] > 0 and np.array_equal(ctx.coverage_depth(t, start, n_win).astype(np.int64), d[start:start + n_win]), (what, t, start)
    finally:
        ctx.close()
    n = len(batch[2]) - 1
    assert got["batches"] == 1 and got["reads_seen"] == n and 0 < got["reads"] < n and got["accumulate_ms"] > 0.0 and got["summary_ms"] > 0.0
    assert sum(c["depth_sum"] for c in got["contigs"]) == got["covered_columns"] and int(got["hist"].sum()) == sum(LENGTHS)
    counted = [r for r in recs if r["mapped"] and (mode == 1 or r["xt"] == "U")]
    assert any(sum(int(k) for k, _ in cu._CIGAR.findall(r["cigar"])) > 64 for r in counted)
    if model == "ss":
        assert got["insertions"] > 0 and got["deleted_columns"] > 0
        assert {r["reverse"] for r in counted if "D" in r["cigar"]} == {False, True}
    if mode == 2:
        assert got["reads"] < sum(1 for r in recs if r["mapped"])


def test_duplicates_count_like_every_other_read(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = du.with_duplicates(mixed_batch(g, 3000, seed=15), 2500, seed=3)
    got = {}
    for collapse in (True, False):
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_collapse_duplicates(collapse)
            ctx.set_coverage(1)
            res = ctx.map_batch(*batch)
            if collapse:
                info = ctx.collapse_info()
                assert info[1] < info[0] == len(batch[2]) - 1
            ctx.hits_to_records(res, *batch, seed=SEED)
            got[collapse] = assert_device_equals_host(ctx, host_of(idx, params, res, 1), f"collapse={collapse}")
        finally:
            ctx.close()
    cu.assert_equal(got[True], got[False])


def test_reads_finished_by_the_host_tail_count(world, monkeypatch):
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", "4294967295")  # every read past the budget leaves for the host
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 3000, seed=25)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_tail_pops(48)
        ctx.set_coverage(2)
        res = ctx.map_batch(*batch)
        assert ctx.tail_info()["reads"] > 100
        ctx.hits_to_records(res, *batch, seed=SEED)
        assert_device_equals_host(ctx, host_of(idx, params, res, 2))
    finally:
        ctx.close()


def _run_pipeline(ctx, idx, params, batches, mode, acc=None, first_read=0):
    """the batches through ctx at pipeline depth 3, each converted once; -> (the host accumulator over the same results, reads so far)"""
    flying, todo = [], list(batches)
    while todo or flying:
        while todo and len(flying) < 3:
            ctx.submit_batch(*todo[0])
            flying.append(todo.pop(0))
        ctx.select_batch(len(flying) - 1)  # the oldest
        b = flying.pop(0)
        res = ctx.fetch()
        seed = int(mapad_amd.lib().mapad_records_seed_at(SEED, first_read))
        ctx.hits_to_records(res, *b, seed=seed)
        acc = host_of(idx, params, res, mode, seed=seed, into=acc)
        first_read += len(b[2]) - 1
    return acc, first_read


def test_batches_in_flight_accumulate_and_two_contexts_merge(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batches = [mixed_batch(g, 1500 + 300 * k, seed=40 + k) for k in range(5)]
    one, a, b = (mapad_amd.Context(idx, params, 0) for _ in range(3))
    try:
        for c in (one, a, b):
            c.set_pipeline_depth(3)
            c.set_coverage(1)
        acc, n = _run_pipeline(one, idx, params, batches, 1)
        got = assert_device_equals_host(one, acc, "five batches at depth 3")
        assert got["batches"] == 5 and got["reads_seen"] == n
        # two contexts that took one half of the batches each, merged: the context that took all
        acc_a, n_a = _run_pipeline(a, idx, params, batches[:2], 1)
        _run_pipeline(b, idx, params, batches[2:], 1, first_read=n_a)
        half = a.coverage()
        assert half["batches"] == 2 and half["reads"] < got["reads"]
        a.merge_coverage(b)
        merged = assert_device_equals_host(a, acc, "merged")
        cu.assert_equal(merged, got, "merged against the one context")
        assert merged["batches"] == 5
        assert b.coverage()["batches"] == 3  # the source keeps its own
        b.set_coverage(2)
        with pytest.raises(mapad_amd.MapadError) as e:  # another mode: not the same table
            a.merge_coverage(b)
        assert e.value.code == -1  # MAPAD_ERR_INVALID
        b.set_coverage(0)
        with pytest.raises(mapad_amd.MapadError) as e:
            a.merge_coverage(b)
        assert e.value.code == -1
    finally:
        for c in (one, a, b):
            c.close()


def _is_zero(cov):
    return (cov["batches"] == 0 and cov["reads_seen"] == 0 and cov["reads"] == 0 and cov["covered_columns"] == 0 and not cov["hist"][1:].any()
            and all(c["reads"] == 0 and c["covered_bases"] == 0 and c["depth_sum"] == 0 and c["max_depth"] == 0 for c in cov["contigs"]) and cov["accumulate_ms"] == 0.0)


def test_a_batch_counts_once_reset_zeroes_and_off_is_off(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 3000, seed=55)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        res = ctx.map_batch(*batch)  # mode 0, the default
        ctx.hits_to_records(res, *batch, seed=SEED)
        off = ctx.coverage()
        assert _is_zero(off) and not off["hist"].any() and not ctx.coverage_depth(0, 100, 1000).any()
        ctx.set_coverage(1)
        res = ctx.map_batch(*batch)
        ctx.hits_to_records(res, *batch, seed=SEED)
        acc = host_of(idx, params, res, 1)
        once = assert_device_equals_host(ctx, acc, "once")
        ctx.hits_to_records(res, *batch, seed=SEED)  # the same result again, then the same batch through mapad_records_device
        ctx.records_device(seed=SEED)
        again = assert_device_equals_host(ctx, acc, "converted three times")
        assert again["batches"] == once["batches"] == 1
        ctx.reset_coverage()
        zero = ctx.coverage()
        assert _is_zero(zero) and int(zero["hist"][0]) == sum(LENGTHS) and not ctx.coverage_depth(1, 0, LENGTHS[1]).any()
        ctx.hits_to_records(res, *batch, seed=SEED)  # nothing has been counted: the batch, still resident, counts into the fresh table
        assert_device_equals_host(ctx, acc, "after the reset")
        ctx.set_coverage(0)
        res = ctx.map_batch(*batch)
        ctx.hits_to_records(res, *batch, seed=SEED)
        assert _is_zero(ctx.coverage())
    finally:
        ctx.close()


def test_uploaded_hits_are_refused_only_while_coverage_is_on(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 1000, seed=65)
    a, b = mapad_amd.Context(idx, params, 0), mapad_amd.Context(idx, params, 0)
    try:
        res = a.map_batch(*batch)
        want = a.hits_to_records(res, *batch, seed=SEED)
        assert b.hits_to_records(res, *batch, seed=SEED) == want  # another context's result: its hits are uploaded
        b.set_coverage(1)
        with pytest.raises(mapad_amd.MapadError) as e:
            b.hits_to_records(res, *batch, seed=SEED)
        assert e.value.code == -9  # MAPAD_ERR_UNSUPPORTED
        assert b.coverage()["batches"] == 0
        b.set_coverage(0)
        assert b.hits_to_records(res, *batch, seed=SEED) == want
    finally:
        a.close()
        b.close()


def test_coverage_and_the_damage_profile_together_equal_their_solo_results(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 3000, seed=75)
    out = {}
    for name, (cov, dmg) in {"both": (2, 1), "coverage": (2, 0), "damage": (0, 1)}.items():
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_coverage(cov)
            ctx.set_damage_profile(dmg)
            res = ctx.map_batch(*batch)
            ctx.hits_to_records(res, *batch, seed=SEED)
            out[name] = (ctx.coverage(), [ctx.coverage_depth(t, 0, n) for t, n in enumerate(LENGTHS)], ctx.damage_profile())
        finally:
            ctx.close()
    cu.assert_equal(out["both"][0], out["coverage"][0])
    assert all(np.array_equal(x, y) for x, y in zip(out["both"][1], out["coverage"][1]))
    du.assert_equal(out["both"][2], out["damage"][2])
    assert out["both"][0]["reads"] > 0 and out["both"][2]["reads"] > out["both"][0]["reads"] and _is_zero(out["damage"][0]) and out["coverage"][2]["batches"] == 0


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def _decoded(path):
    text, refs, recs = read_bam(path)
    out = []
    for r in recs:
        tags = {k: v for k, v in r["tags"].items() if k != "XD"}  # (XD: wall time per read)
        out.append((r["name"], r["flags"], r["tid"], r["pos"], r["mapq"], r["bin"], r["cigar"], r["seq"], r["qual"], tuple(sorted(tags.items())), tuple(r["tag_order"])))
    return re.sub(r"\tCL:[^\t\n]*", "", text), refs, out  # (CL: the command line, which names the flag and the output file)


def _read_tsv(path):
    """-> (the first line's fields, the per-contig rows as the table's dicts + name, hist); the printed percentages checked against the integer columns"""
    lines = open(path).read().splitlines()
    assert lines[0].startswith("#mapad-amd-coverage v1 ")
    head = dict(kv.split("=") for kv in lines[0].split()[2:])
    assert list(head) == ["mode", "reads", "reads_seen", "contigs", "bins"] and head["bins"] == "256"
    assert lines[1] == "#rname\tstartpos\tendpos\tnumreads\tcovbases\tcoverage\tmeandepth\tmaxdepth"
    nc = int(head["contigs"])
    rows = []
    for ln in lines[2:2 + nc]:
        f = ln.split("\t")
        assert len(f) == 8 and f[1] == "1"
        length, reads, covered, max_depth = int(f[2]), int(f[3]), int(f[4]), int(f[7])
        assert f[5] == "%.4f" % (100.0 * covered / length)
        rows.append({"name": f[0], "length": length, "reads": reads, "covered_bases": covered, "meandepth": f[6], "max_depth": max_depth})
    assert lines[2 + nc] == "#depth\tbases" and len(lines) == 3 + nc + 256
    hist = np.zeros(256, np.uint64)
    for d, ln in enumerate(lines[3 + nc:]):
        f = ln.split("\t")
        assert int(f[0]) == d
        hist[d] = int(f[1])
    return head, rows, hist


def test_cli_writes_the_coverage_of_the_bam_it_wrote(tmp_path):
    """The BAM of a run with --coverage holds the same records as one without: every field, tag and the tag order — all but the XD tag (wall time) and the header's
    CL field (the command line itself), which differ between any two runs."""
    mapad_amd.lib()
    cli = mbuild.build_cli()
    g = synth.genome(120_000, seed=17)
    g[90_000:90_300] = g[30_000:30_300]
    split = 70_003
    fa, fq = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fastq")
    with open(fa, "w") as f:
        for name, s in (("chr1", g[:split].tobytes().decode()), ("chr2", g[split:].tobytes().decode())):
            f.write(f">{name}\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    lengths = [split, 120_000 - split]
    u = synth.reads(g, 3000, seed=23, qual_range=(20, 23), damage=DMG, len_range=(25, 110), indel_frac=0.3)
    rep = synth.reads(g[30_000:30_300], 200, 40, seed=24, qual_range=(20, 23), exo_frac=0.0)
    edges = cu.hand_made([g[0:40], g[split:split + 40], g[split - 40:split], g[120_000 - 40:120_000]], qual=22)
    seqs, quals, offsets = du.with_duplicates(cu.concat(u, rep, edges), 2296, seed=13)
    with open(fq, "w") as f:
        for i in range(len(offsets) - 1):
            s, e = int(offsets[i]), int(offsets[i + 1])
            f.write(f"@r{i}\n{seqs[s:e].tobytes().decode()}\n+\n{''.join(chr(33 + q) for q in quals[s:e])}\n")
    subprocess.check_call(GUARD + [cli, "index", "-g", fa])
    base = GUARD + [cli, "map", "-r", fq, "-g", fa, "-l", "single_stranded", "-p", "0.03", "-f", "0.5", "-t", "0.5", "-d", "0.02", "-s", "1.0", "-i", "0.001", "--seed", "7",
                    "--batch_size", "1000"]
    subprocess.check_call(base + ["-o", str(tmp_path / "plain.bam")])
    plain = _decoded(str(tmp_path / "plain.bam"))
    assert len(plain[2]) == 5500

    def check(name, extra, mode, env=None):
        bam, tsv = str(tmp_path / f"{name}.bam"), str(tmp_path / f"{name}.tsv")
        pr = subprocess.run(base + ["-o", bam, "--coverage", tsv] + extra, check=True, stderr=subprocess.PIPE, text=True, env=env)
        assert "coverage (%s)" % ("unique" if mode == 2 else "all") in pr.stderr and "bases covered, mean depth" in pr.stderr, pr.stderr
        assert _decoded(bam) == plain, name
        want = cu.from_bam(lengths, read_bam(bam)[2], mode)
        head, rows, hist = _read_tsv(tsv)
        assert head["mode"] == ("unique" if mode == 2 else "all") and int(head["reads"]) == want["reads"] and int(head["reads_seen"]) == want["reads_seen"] == 5500
        assert [r["name"] for r in rows] == ["chr1", "chr2"] == [r[0] for r in plain[1]]
        for r, w in zip(rows, want["contigs"]):
            for k in ("length", "reads", "covered_bases", "max_depth"):
                assert r[k] == w[k], (name, k, r, w)
            assert r["meandepth"] == "%.6f" % (w["depth_sum"] / w["length"]), (name, r, w)
        assert np.array_equal(hist, want["hist"]), name
        assert want["reads"] > 0 and want["insertions"] > 0 and want["deleted_columns"] > 0 and all(d[0] > 0 and d[-1] > 0 for d in want["depth"])
        return head, rows, hist

    all_run = check("all", [], 1)
    check("all_collapsed", ["--collapse_duplicates"], 1)
    unique = check("unique_coalesced", ["--coverage_unique", "--coalesce", "2"], 2)
    assert int(unique[0]["reads"]) < int(all_run[0]["reads"])
    # The repair path of the chunk loop: hit pools too small for a chunk (MAPAD_HIT_POOL, the library's test hook) make the fetches of the chunks in flight fail; they
    # are re-run one by one, over batch slots that hold collected chunks.  Same records with and without coverage, and no chunk goes uncounted or counts twice.
    small = dict(os.environ, MAPAD_HIT_POOL="64")
    subprocess.check_call(base + ["-o", str(tmp_path / "small.bam")], env=small)
    assert _decoded(str(tmp_path / "small.bam")) == plain
    repaired = check("small_all", [], 1, env=small)
    assert repaired[0] == all_run[0] and repaired[1] == all_run[1] and np.array_equal(repaired[2], all_run[2])
    # coverage and the damage profile in one run: each file as in its own run
    bam, tsv, dmg = str(tmp_path / "both.bam"), str(tmp_path / "both.tsv"), str(tmp_path / "both_damage.tsv")
    subprocess.check_call(base + ["-o", bam, "--coverage", tsv, "--damage_profile", dmg])
    assert _decoded(bam) == plain and open(tsv).read() == open(str(tmp_path / "all.tsv")).read()
