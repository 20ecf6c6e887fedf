"""The damage profile on the GPU (run with -m gpu on an MI355X): what damage_kernel accumulates in a context while batches are converted to records equals
mapad_damage_profile_host over the same fetched results and seeds, counter for counter — under every path a batch can take (both search kernels, duplicate
collapsing, reads finished by the host tail, batches in flight, the CLI) — and equals the table decoded independently from the records / the BAM
(tests/damage_util.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import build as mbuild
from mapad_amd import synth

import damage_util as du
from damage_util import with_duplicates
from bam_util import read_bam
from kat_util import resolve_params
from parity_util import DAMAGE, DOUBLE_STRANDED

pytestmark = pytest.mark.gpu

DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 99
# TestDifferenceModel + TestBound: the alignment starts in the middle of the read, so the general-direction search step runs and the operations of a track are not
# in read order
TEST_MODEL = {"model": "test", "deam_score": -0.5, "mm_score": -1.0, "match_score": 0.0, "bound": "test", "threshold": -2.0, "repr_mm_bound": -1.0,
              "penalty_gap_open": -2.0, "penalty_gap_extend": -1.0, "gap_dist_ends": 5, "max_num_gaps_open": 1}
MODELS = {"ss": DAMAGE, "ds": DOUBLE_STRANDED, "test_model": TEST_MODEL}
GUARD = ["timeout", "-k", "10", "600"]  # every GPU child process under a time limit of its own


@pytest.fixture(scope="module")
def world():
    g = synth.genome(400_000, seed=77)
    g[300_000:300_400] = g[100_000:100_400]  # a repeat: reads from it have X0 > 1 (mode 2 leaves them out)
    return g, mapad_amd.Index.build([("c1", g[:250_000]), ("c2", g[250_000:])])


def mixed_batch(g, n, seed):
    a = synth.reads(g, n, seed=seed, qual_range=(20, 40), damage=DMG, len_range=(20, 70), indel_frac=0.2)
    b = synth.reads(g[100_000:100_400], n // 10, 45, seed=seed + 1, exo_frac=0.0, damage=DMG)
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2][1:] + a[2][-1]])


def convert_and_compare(ctx, idx, params, batch, res, mode, seed=SEED, into=None):
    """records on the device (which adds the batch to the context's profile) -> the host path over the same result, added to `into`"""
    recs = ctx.hits_to_records(res, *batch, seed=seed)
    want = mb.damage_profile_host(idx, params, res, batch[0], batch[2], seed=seed, mode=mode, into=into)
    return recs, want


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("model", list(MODELS))
def test_device_profile_equals_the_host_path(world, model, mode):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(MODELS[model]))
    batch = mixed_batch(g, 6000, seed=5)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_damage_profile(mode)
        res = ctx.map_batch(*batch)
        recs, want = convert_and_compare(ctx, idx, params, batch, res, mode)
        got = ctx.damage_profile()
    finally:
        ctx.close()
    du.assert_equal(got, want, model)
    du.assert_equal(got, du.from_records(recs, batch[0], batch[2], mode), model + ": numpy table from the device's records")
    n = len(batch[2]) - 1
    assert got["batches"] == 1 and got["reads_seen"] == n and 0 < got["reads"] < n and got["kernel_ms"] > 0.0
    assert int(got["counts"][0].sum()) <= got["aligned_bases"]
    if model != "test_model":
        assert got["insertions"] > 0 and got["deletions"] > 0
    if mode == 2:
        assert got["reads"] < sum(1 for r in recs if r["mapped"])


def test_duplicates_count_like_every_other_read(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = with_duplicates(mixed_batch(g, 5000, seed=15), 4000, seed=3)
    got = {}
    for collapse in (True, False):
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_collapse_duplicates(collapse)
            ctx.set_damage_profile(1)
            res = ctx.map_batch(*batch)
            if collapse:
                info = ctx.collapse_info()
                assert info[1] < info[0] == len(batch[2]) - 1
            _, want = convert_and_compare(ctx, idx, params, batch, res, 1)
            got[collapse] = ctx.damage_profile()
            du.assert_equal(got[collapse], want, f"collapse={collapse}")
        finally:
            ctx.close()
    du.assert_equal(got[True], got[False])


def test_reads_finished_by_the_host_tail_count(world, monkeypatch):
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", "4294967295")  # every read past the budget leaves for the host
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 3000, seed=25)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_tail_pops(48)
        ctx.set_damage_profile(2)
        res = ctx.map_batch(*batch)
        assert ctx.tail_info()["reads"] > 100
        _, want = convert_and_compare(ctx, idx, params, batch, res, 2)
        du.assert_equal(ctx.damage_profile(), want)
    finally:
        ctx.close()


def test_batches_in_flight_accumulate(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batches = [mixed_batch(g, 1500 + 300 * k, seed=40 + k) for k in range(5)]
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_pipeline_depth(3)
        ctx.set_damage_profile(1)
        want, flying, first_read = None, [], 0
        todo = list(batches)
        while todo or flying:
            while todo and len(flying) < 3:
                ctx.submit_batch(*todo[0])
                flying.append(todo.pop(0))
            ctx.select_batch(len(flying) - 1)  # the oldest
            b = flying.pop(0)
            res = ctx.fetch()
            seed = int(mapad_amd.lib().mapad_records_seed_at(SEED, first_read))
            _, want = convert_and_compare(ctx, idx, params, b, res, 1, seed=seed, into=want)
            first_read += len(b[2]) - 1
        got = ctx.damage_profile()
    finally:
        ctx.close()
    du.assert_equal(got, want)
    assert got["batches"] == want["batches"] == 5 and got["reads_seen"] == first_read


def test_a_batch_counts_once_reset_zeroes_and_off_is_off(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 3000, seed=55)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        res = ctx.map_batch(*batch)  # mode 0, the default
        ctx.hits_to_records(res, *batch, seed=SEED)
        off = ctx.damage_profile()
        assert off["batches"] == 0 and off["reads_seen"] == 0 and off["reads"] == 0 and off["aligned_bases"] == 0 and not off["counts"].any() and off["kernel_ms"] == 0.0
        ctx.set_damage_profile(1)
        res = ctx.map_batch(*batch)
        _, want = convert_and_compare(ctx, idx, params, batch, res, 1)
        once = ctx.damage_profile()
        ctx.hits_to_records(res, *batch, seed=SEED)  # the same result again, then the same batch through mapad_records_device
        ctx.records_device(seed=SEED)
        again = ctx.damage_profile()
        du.assert_equal(once, want)
        du.assert_equal(again, once)
        assert again["batches"] == 1
        ctx.reset_damage_profile()
        zero = ctx.damage_profile()
        assert zero["batches"] == 0 and zero["reads_seen"] == 0 and not zero["counts"].any() and zero["kernel_ms"] == 0.0
        ctx.hits_to_records(res, *batch, seed=SEED)  # nothing has been counted: the batch, still resident, counts into the fresh table
        du.assert_equal(ctx.damage_profile(), want)
        ctx.set_damage_profile(0)
        res = ctx.map_batch(*batch)
        ctx.hits_to_records(res, *batch, seed=SEED)
        assert ctx.damage_profile()["batches"] == 0
    finally:
        ctx.close()


def test_uploaded_hits_are_refused_only_while_the_profile_is_on(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 1000, seed=65)
    a, b = mapad_amd.Context(idx, params, 0), mapad_amd.Context(idx, params, 0)
    try:
        res = a.map_batch(*batch)
        want = a.hits_to_records(res, *batch, seed=SEED)
        assert b.hits_to_records(res, *batch, seed=SEED) == want  # another context's result: its hits are uploaded
        b.set_damage_profile(1)
        with pytest.raises(mapad_amd.MapadError) as e:
            b.hits_to_records(res, *batch, seed=SEED)
        assert e.value.code == -9  # MAPAD_ERR_UNSUPPORTED
        assert b.damage_profile()["batches"] == 0
        b.set_damage_profile(0)
        assert b.hits_to_records(res, *batch, seed=SEED) == want
    finally:
        a.close()
        b.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def _decoded(path):
    text, refs, recs = read_bam(path)
    out = []
    for r in recs:
        tags = {k: v for k, v in r["tags"].items() if k != "XD"}  # (XD: wall time per read)
        out.append((r["name"], r["flags"], r["tid"], r["pos"], r["mapq"], r["bin"], r["cigar"], r["seq"], r["qual"], tuple(sorted(tags.items())), tuple(r["tag_order"])))
    return re.sub(r"\tCL:[^\t\n]*", "", text), refs, out  # (CL: the command line, which names the flag and the output file)


def _read_tsv(path):
    lines = open(path).read().splitlines()
    head = dict(kv.split("=") for kv in lines[0].split()[2:])
    assert lines[0].startswith("#mapad-amd-damage-profile v1 ") and head["positions"] == "32"
    cols = lines[1].split("\t")
    assert cols == ["end", "pos"] + [f"{r}>{q}" for r in "ACGT" for q in "ACGT"] + ["C>T_freq", "G>A_freq"]
    assert len(lines) == 2 + 64
    counts = np.zeros((2, 32, 4, 4), np.uint64)
    for k, ln in enumerate(lines[2:]):
        f = ln.split("\t")
        e, p = k // 32, k % 32
        assert f[0] == ("5p", "3p")[e] and int(f[1]) == p + 1
        counts[e, p] = np.array([int(x) for x in f[2:18]], np.uint64).reshape(4, 4)
        for txt, r, q in ((f[18], 1, 3), (f[19], 2, 0)):
            den = int(counts[e, p, r].sum())
            assert txt == ("%.6f" % (int(counts[e, p, r, q]) / den if den else 0.0))
    return head, counts


def test_cli_writes_the_profile_of_the_bam_it_wrote(tmp_path):
    """The BAM of a run with --damage_profile holds the same records as one without: every field, tag and the tag order — all but the XD tag (wall time) and the
    header's CL field (the command line itself), which differ between any two runs."""
    mapad_amd.lib()
    cli = mbuild.build_cli()
    g = synth.genome(120_000, seed=17)
    g[90_000:90_300] = g[30_000:30_300]
    fa, fq = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fastq")
    with open(fa, "w") as f:
        f.write(">chr1\n")
        s = g.tobytes().decode()
        for i in range(0, len(s), 60):
            f.write(s[i:i + 60] + "\n")
    u = synth.reads(g, 3000, seed=23, qual_range=(20, 23), damage=DMG, len_range=(25, 80), indel_frac=0.2)
    rep = synth.reads(g[30_000:30_300], 200, 40, seed=24, qual_range=(20, 23), exo_frac=0.0)
    seqs, quals, offsets = with_duplicates((np.concatenate([u[0], rep[0]]), np.concatenate([u[1], rep[1]]), np.concatenate([u[2], rep[2][1:] + u[2][-1]])), 2300, seed=13)
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
    runs = {"all": ([], 1), "all_collapsed": (["--collapse_duplicates"], 1), "unique_coalesced": (["--damage_profile_unique", "--coalesce", "2"], 2)}
    for name, (extra, mode) in runs.items():
        bam, tsv = str(tmp_path / f"{name}.bam"), str(tmp_path / f"{name}.tsv")
        pr = subprocess.run(base + ["-o", bam, "--damage_profile", tsv] + extra, check=True, stderr=subprocess.PIPE, text=True)
        assert "damage profile (%s)" % ("unique" if mode == 2 else "all") in pr.stderr and "C>T at 5p pos 1" in pr.stderr, pr.stderr
        assert _decoded(bam) == plain, name
        want = du.from_bam(read_bam(bam)[2], mode)
        head, counts = _read_tsv(tsv)
        assert np.array_equal(counts, want["counts"]), name
        assert head["mode"] == ("unique" if mode == 2 else "all") and int(head["reads"]) == want["reads"] and int(head["reads_seen"]) == want["reads_seen"] == 5500
        assert want["reads"] > 0 and want["insertions"] + want["deletions"] > 0
    assert int(_read_tsv(str(tmp_path / "unique_coalesced.tsv"))[0]["reads"]) < int(_read_tsv(str(tmp_path / "all.tsv"))[0]["reads"])
    # The repair path of the chunk loop: hit pools too small for a chunk (MAPAD_HIT_POOL, the library's test hook) make the fetches of the chunks in flight fail; they
    # are re-run one by one, over batch slots that hold collected chunks.  Same records with and without the profile, and no chunk goes uncounted.
    small = dict(os.environ, MAPAD_HIT_POOL="64")
    subprocess.check_call(base + ["-o", str(tmp_path / "small.bam")], env=small)
    assert _decoded(str(tmp_path / "small.bam")) == plain
    bam, tsv = str(tmp_path / "small_all.bam"), str(tmp_path / "small_all.tsv")
    subprocess.check_call(base + ["-o", bam, "--damage_profile", tsv], env=small)
    assert _decoded(bam) == plain
    head, counts = _read_tsv(tsv)
    all_head, all_counts = _read_tsv(str(tmp_path / "all.tsv"))
    assert np.array_equal(counts, all_counts) and head == all_head
