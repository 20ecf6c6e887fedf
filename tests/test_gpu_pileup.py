"""The pileup on the GPU (run with -m gpu on an MI355X): what pileup_kernel accumulates in a context while batches are converted to records, and what
pileup_call_kernel makes of it, equals mapad_pileup_host_* over the same fetched results, reads and seeds — scalars, per-contig statistics, raw counts and
consensus — under every path a batch can take (both search steps, duplicate collapsing, reads finished by the host tail, batches in flight, two contexts merged,
the CLI), and equals the table built independently in numpy from the records / the BAM (tests/pileup_util.py)."""
import re
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import build as mbuild
from mapad_amd import synth

import damage_util as du
import pileup_util as pu
from bam_util import read_bam
from kat_util import resolve_params
from parity_util import DAMAGE

pytestmark = pytest.mark.gpu

DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 99
# TestDifferenceModel + TestBound: the alignment starts in the middle of the read, so the general-direction search step runs and the operations of a track are not
# in read order.  (Its threshold of -2 admits no gap — opening one costs -3 —, so insertions and deletions are asserted for "ss" only.)
TEST_MODEL = {"model": "test", "deam_score": -0.5, "mm_score": -1.0, "match_score": 0.0, "bound": "test", "threshold": -2.0, "repr_mm_bound": -1.0,
              "penalty_gap_open": -2.0, "penalty_gap_extend": -1.0, "gap_dist_ends": 5, "max_num_gaps_open": 1}
MODELS = {"ss": DAMAGE, "test_model": TEST_MODEL}
GUARD = ["timeout", "-k", "10", "600"]  # every GPU child process under a time limit of its own
SPLIT = 250_007
LENGTHS = [SPLIT, 400_000 - SPLIT]
FILTERS = [(0, 0, 0), (30, 3, 2)]  # (min_bq, mask5, mask3)
RULE = (3, 80)                     # (min_depth, min_percent) of most summaries here; (1, 0) beside it


@pytest.fixture(scope="module")
def world():
    g = synth.genome(400_000, seed=77)
    g[300_000:300_400] = g[100_000:100_400]  # a repeat: reads from it have X0 > 1 (mode 2 leaves them out)
    return g, mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])


def with_n(read, at):
    read = read.copy()
    read[at] = ord("N")
    return read


def mixed_batch(g, n, seed):
    """reads of 20..150 bases with indels (tracks longer than a wavefront, deletions on both strands), reads from the repeat, reads on the contigs' first and last
    bases, and reads with an N on either strand"""
    edges = pu.hand_made([g[0:40], g[SPLIT:SPLIT + 40], g[SPLIT - 40:SPLIT], g[400_000 - 40:400_000], synth.revcomp(g[SPLIT - 45:SPLIT]), with_n(g[16_360:16_410], 20),
                          with_n(synth.revcomp(g[SPLIT + 40:SPLIT + 90]), 31), with_n(g[50_000:50_120], 100)])
    return pu.concat(synth.reads(g, n, seed=seed, qual_range=(20, 40), damage=DMG, len_range=(20, 150), indel_frac=0.3),
                     synth.reads(g[100_000:100_400], n // 10, 45, seed=seed + 1, exo_frac=0.0, damage=DMG), edges)


def host_of(idx, params, res, batch, mode, flt=(0, 0, 0), seed=SEED, into=None):
    return (into if into is not None else mb.PileupHost(idx, mode, *flt)).add(params, res, *batch, seed=seed)


def assert_device_equals_host(ctx, acc, what="", rules=(RULE,)):
    for rule in rules:
        got = ctx.pileup(*rule)
        pu.assert_equal(got, acc.summary(*rule), *rule, what=f"{what}, rule {rule}")
        for t, n in enumerate(LENGTHS):
            assert np.array_equal(ctx.pileup_counts(t, 0, n), acc.counts(t, 0, n)), (what, "counts of contig", t)
            assert np.array_equal(ctx.pileup_consensus(t, 0, n, *rule), acc.consensus(t, 0, n, *rule)), (what, rule, "consensus of contig", t)
    return got


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("model", list(MODELS))
def test_device_pileup_equals_the_host_path_and_the_records(world, model, mode):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(MODELS[model]))
    batch = mixed_batch(g, 5000, seed=5)
    n = len(batch[2]) - 1
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_pileup(mode, *FILTERS[0])
        res = ctx.map_batch(*batch)
        for flt in FILTERS:
            ctx.set_pileup(mode, *flt)  # (a change of the filters starts an empty table: the batch, still resident, counts into it)
            recs = ctx.hits_to_records(res, *batch, seed=SEED)
            what = f"{model}, mode {mode}, filters {flt}"
            got = assert_device_equals_host(ctx, host_of(idx, params, res, batch, mode, flt), what, rules=(RULE, (1, 0)))
            want = pu.from_records(LENGTHS, recs, batch, mode, *flt)
            pu.assert_equal(ctx.pileup(*RULE), want, *RULE, what=what + ": numpy table from the device's records", counts_of=ctx.pileup_counts, consensus_of=ctx.pileup_consensus)
            for t, c in enumerate(want["counts"]):  # windows that start in the middle of a contig, on covered ground
                d = c.sum(axis=1)
                for start in (int(np.argmax(d)), LENGTHS[t] - 30):
                    k = min(5000, LENGTHS[t] - start)
                    assert d[start] > 0 and np.array_equal(ctx.pileup_counts(t, start, k).astype(np.int64), c[start:start + k]), (what, t, start)
                    assert np.array_equal(ctx.pileup_consensus(t, start, k, 2, 60), pu.consensus(c[start:start + k], 2, 60)), (what, t, start)
            assert got["batches"] == 1 and got["reads_seen"] == n and 0 < got["reads"] < n and got["accumulate_ms"] > 0.0 and got["summary_ms"] > 0.0
            assert (got["mode"], got["min_base_quality"], got["mask5"], got["mask3"]) == (mode,) + flt
            assert got["columns_not_acgt"] > 0 and all(c["sites_called"] > 0 for c in got["contigs"])
            if flt != (0, 0, 0):
                assert got["columns_masked"] > 0 and got["columns_low_quality"] > 0
            else:
                assert got["columns_masked"] == 0 and got["columns_low_quality"] == 0
    finally:
        ctx.close()
    counted = [r for r in recs if r["mapped"] and (mode == 1 or r["xt"] == "U")]
    assert any(sum(int(k) for k, _ in pu._CIGAR.findall(r["cigar"])) > 64 for r in counted)
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
            ctx.set_pileup(1, 30, 3, 2)
            res = ctx.map_batch(*batch)
            if collapse:
                info = ctx.collapse_info()
                assert info[1] < info[0] == len(batch[2]) - 1
            ctx.hits_to_records(res, *batch, seed=SEED)
            got[collapse] = (assert_device_equals_host(ctx, host_of(idx, params, res, batch, 1, (30, 3, 2)), f"collapse={collapse}"),
                             [ctx.pileup_counts(t, 0, n) for t, n in enumerate(LENGTHS)])
        finally:
            ctx.close()
    pu.assert_equal(got[True][0], got[False][0], *RULE)
    assert all(np.array_equal(x, y) for x, y in zip(got[True][1], got[False][1]))


def test_reads_finished_by_the_host_tail_count(world, monkeypatch):
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", "4294967295")  # every read past the budget leaves for the host
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 3000, seed=25)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_tail_pops(48)
        ctx.set_pileup(2, 25, 2, 2)
        res = ctx.map_batch(*batch)
        assert ctx.tail_info()["reads"] > 100
        ctx.hits_to_records(res, *batch, seed=SEED)
        assert_device_equals_host(ctx, host_of(idx, params, res, batch, 2, (25, 2, 2)))
    finally:
        ctx.close()


def _run_pipeline(ctx, idx, params, batches, mode, flt, acc=None, first_read=0):
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
        acc = host_of(idx, params, res, b, mode, flt, seed=seed, into=acc)
        first_read += len(b[2]) - 1
    return acc, first_read


def test_batches_in_flight_accumulate_and_two_contexts_merge(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batches = [mixed_batch(g, 1500 + 300 * k, seed=40 + k) for k in range(5)]
    flt = (30, 3, 2)
    one, a, b = (mapad_amd.Context(idx, params, 0) for _ in range(3))
    try:
        for c in (one, a, b):
            c.set_pipeline_depth(3)
            c.set_pileup(1, *flt)
        acc, n = _run_pipeline(one, idx, params, batches, 1, flt)
        got = assert_device_equals_host(one, acc, "five batches at depth 3")
        assert got["batches"] == 5 and got["reads_seen"] == n
        # two contexts that took one half of the batches each, merged: the context that took all
        _, n_a = _run_pipeline(a, idx, params, batches[:2], 1, flt)
        _run_pipeline(b, idx, params, batches[2:], 1, flt, first_read=n_a)
        half = a.pileup(*RULE)
        assert half["batches"] == 2 and half["reads"] < got["reads"]
        a.pileup_merge(b)
        merged = assert_device_equals_host(a, acc, "merged")
        pu.assert_equal(merged, got, *RULE, what="merged against the one context")
        assert merged["batches"] == 5
        assert b.pileup(*RULE)["batches"] == 3  # the source keeps its own
        for other in ((1, 30, 3, 1), (1, 29, 3, 2), (1, 30, 0, 2), (2, 30, 3, 2), (0, 0, 0, 0)):  # another filter, another mode, off: not the same table
            b.set_pileup(*other)
            with pytest.raises(mapad_amd.MapadError) as e:
                a.pileup_merge(b)
            assert e.value.code == -1  # MAPAD_ERR_INVALID
        with pytest.raises(mapad_amd.MapadError) as e:
            a.pileup_merge(a)
        assert e.value.code == -1
        pu.assert_equal(a.pileup(*RULE), got, *RULE, what="after the refused merges")
    finally:
        for c in (one, a, b):
            c.close()


def _is_zero(p):
    return (p["batches"] == 0 and all(p[k] == 0 for k in pu.SCALARS) and p["accumulate_ms"] == 0.0
            and all(c["sites_covered"] == 0 and c["sites_deep"] == 0 and c["sites_called"] == 0 and c["max_depth"] == 0 and not any(c["called"]) and not any(c["base_sum"])
                    for c in p["contigs"]))


def _error_of(call):
    try:
        call()
    except mapad_amd.MapadError as e:
        return e.code
    return None


def test_a_batch_counts_once_reset_zeroes_and_off_is_off(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 3000, seed=55)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        res_off = ctx.map_batch(*batch)  # mode 0, the default
        recs_off = ctx.hits_to_records(res_off, *batch, seed=SEED)
        off = ctx.pileup(1, 0)
        assert _is_zero(off) and off["mode"] == 0 and [c["length"] for c in off["contigs"]] == LENGTHS
        assert _error_of(lambda: ctx.pileup(1, 0)) == _error_of(ctx.coverage)  # what coverage() answers on a context where it is off: the same here
        assert not ctx.pileup_counts(0, 100, 1000).any() and bytes(ctx.pileup_consensus(1, 0, 4)) == b"NNNN"
        ctx.set_pileup(1)
        res = ctx.map_batch(*batch)
        recs = ctx.hits_to_records(res, *batch, seed=SEED)
        # off and on: the same results and the same records, byte for byte
        assert recs == recs_off and np.array_equal(res.hit_begin, res_off.hit_begin) and np.array_equal(res.ops, res_off.ops)
        assert all(res.hits_arr[k].tobytes() == res_off.hits_arr[k].tobytes() for k in ("lower", "lower_rev", "size", "score", "n_ops", "ops_offset"))
        acc = host_of(idx, params, res, batch, 1)
        once = assert_device_equals_host(ctx, acc, "once")
        ctx.hits_to_records(res, *batch, seed=SEED)  # the same result again, then the same batch through mapad_records_device
        ctx.records_device(seed=SEED)
        again = assert_device_equals_host(ctx, acc, "converted three times")
        assert again["batches"] == once["batches"] == 1
        ctx.pileup_reset()
        zero = ctx.pileup(*RULE)
        assert _is_zero(zero) and zero["mode"] == 1 and not ctx.pileup_counts(1, 0, LENGTHS[1]).any()
        ctx.hits_to_records(res, *batch, seed=SEED)  # nothing has been counted: the batch, still resident, counts into the fresh table
        assert_device_equals_host(ctx, acc, "after the reset")
        ctx.set_pileup(0)
        res = ctx.map_batch(*batch)
        ctx.hits_to_records(res, *batch, seed=SEED)
        assert _is_zero(ctx.pileup(1, 0))
        for bad in (lambda: ctx.pileup(0, 0), lambda: ctx.pileup(1, 101), lambda: ctx.pileup_consensus(0, 0, 4, 0, 0), lambda: ctx.pileup_counts(0, LENGTHS[0] - 3, 4),
                    lambda: ctx.pileup_counts(2, 0, 1), lambda: ctx.set_pileup(3), lambda: ctx.set_pileup(1, 256), lambda: ctx.set_pileup(1, 0, 65536)):
            assert _error_of(bad) == -1  # MAPAD_ERR_INVALID
    finally:
        ctx.close()


def test_uploaded_hits_are_refused_only_while_the_pileup_is_on(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 1000, seed=65)
    a, b = mapad_amd.Context(idx, params, 0), mapad_amd.Context(idx, params, 0)
    try:
        res = a.map_batch(*batch)
        want = a.hits_to_records(res, *batch, seed=SEED)
        assert b.hits_to_records(res, *batch, seed=SEED) == want  # another context's result: its hits are uploaded, its reads are not on the device
        b.set_pileup(1)
        with pytest.raises(mapad_amd.MapadError) as e:
            b.hits_to_records(res, *batch, seed=SEED)
        assert e.value.code == -9  # MAPAD_ERR_UNSUPPORTED
        assert b.pileup(1, 0)["batches"] == 0
        b.set_pileup(0)
        assert b.hits_to_records(res, *batch, seed=SEED) == want
    finally:
        a.close()
        b.close()


def test_planted_variants_show_in_the_consensus(world):
    """Reads drawn from a copy of 20 kbp of the genome that differs from it in one base of 997, mapped to the original: the consensus over the stretch is the copy
    wherever there is a call, and there is one at 90 % of the positions at least (a condition the numpy table alone meets: tests/test_pileup_host.py checks it
    through the host path, without a GPU)."""
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    copy, at, batch = pu.planted(g)
    reference = g[pu.PLANT_START:pu.PLANT_START + pu.PLANT_LEN]
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_pileup(1)
        res = ctx.map_batch(*batch)
        recs = ctx.hits_to_records(res, *batch, seed=SEED)
        cons = ctx.pileup_consensus(0, pu.PLANT_START, pu.PLANT_LEN, 3, 80)
        want = pu.from_records(LENGTHS, recs, batch, 1)
        assert np.array_equal(cons, pu.consensus(want["counts"][0][pu.PLANT_START:pu.PLANT_START + pu.PLANT_LEN], 3, 80))
        pu.assert_planted(copy, at, cons, reference)
        # with the reference's own reads the same sites show the reference's base
        ctx.pileup_reset()
        plain = synth.reads(reference, 4000, 50, seed=6, subst_rate=0.01, exo_frac=0.0, qual_range=(20, 40), damage=None)
        res = ctx.map_batch(*plain)
        ctx.hits_to_records(res, *plain, seed=SEED)
        cons = ctx.pileup_consensus(0, pu.PLANT_START, pu.PLANT_LEN, 3, 80)
        called = cons != ord("N")
        assert np.array_equal(cons[called], reference[called]) and called[at].any()
    finally:
        ctx.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def _decoded(path):
    text, refs, recs = read_bam(path)
    out = []
    for r in recs:
        tags = {k: v for k, v in r["tags"].items() if k != "XD"}  # (XD: wall time per read)
        out.append((r["name"], r["flags"], r["tid"], r["pos"], r["mapq"], r["bin"], r["cigar"], r["seq"], r["qual"], tuple(sorted(tags.items())), tuple(r["tag_order"])))
    return re.sub(r"\tCL:[^\t\n]*", "", text), refs, out  # (CL: the command line, which names the options and the output files)


def _read_tsv(path):
    """-> (the first line's fields, the scalars, the per-contig rows as the summary's dicts)"""
    lines = open(path).read().splitlines()
    assert lines[0].startswith("#mapad-amd-pileup v1 ")
    head = dict(kv.split("=") for kv in lines[0].split()[2:])
    assert list(head) == ["mode", "min_bq", "mask5", "mask3", "min_depth", "min_percent", "contigs"]
    names = lines[1][1:].split("\t")
    assert names == list(pu.SCALARS) + ["batches"] and lines[1][0] == "#"
    scalars = dict(zip(names, (int(x) for x in lines[2].split("\t"))))
    assert lines[3] == "#rname\tlength\tsites_covered\tsites_deep\tsites_called\tcalled_A\tcalled_C\tcalled_G\tcalled_T\tsum_A\tsum_C\tsum_G\tsum_T\tmaxdepth"
    rows = []
    for ln in lines[4:]:
        f = ln.split("\t")
        assert len(f) == 14
        v = [int(x) for x in f[1:]]
        rows.append({"name": f[0], "length": v[0], "sites_covered": v[1], "sites_deep": v[2], "sites_called": v[3], "called": v[4:8], "base_sum": v[8:12], "max_depth": v[12]})
    assert len(rows) == int(head["contigs"])
    return head, scalars, rows


def _read_fasta(path):
    """-> [(name, sequence as uint8)]; every line but a record's last has 60 columns"""
    out = []
    for block in open(path).read().split(">")[1:]:
        lines = block.splitlines()
        assert all(len(ln) == 60 for ln in lines[1:-1]) and 0 < len(lines[-1]) <= 60
        out.append((lines[0], np.frombuffer("".join(lines[1:]).encode(), np.uint8)))
    return out


def test_cli_writes_the_pileup_and_the_consensus_of_the_bam_it_wrote(tmp_path):
    """The BAM of a run with --pileup / --consensus holds the same records as one without: every field, tag and the tag order — all but the XD tag (wall time) and the
    header's CL field (the command line itself), which differ between any two runs.  The TSV and the FASTA equal the numpy table of that BAM and what the binding
    gives for the same reads, parameters and seed."""
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
    u = synth.reads(g, 3000, seed=23, qual_range=(20, 40), damage=DMG, len_range=(25, 110), indel_frac=0.3)
    rep = synth.reads(g[30_000:30_300], 200, 40, seed=24, qual_range=(20, 40), exo_frac=0.0)
    edges = pu.hand_made([g[0:40], g[split:split + 40], g[split - 40:split], g[120_000 - 40:120_000], with_n(g[5_000:5_060], 30)], qual=31)
    batch = du.with_duplicates(pu.concat(u, rep, edges), 1295, seed=13)
    seqs, quals, offsets = batch
    n_reads = len(offsets) - 1
    with open(fq, "w") as f:
        for i in range(n_reads):
            s, e = int(offsets[i]), int(offsets[i + 1])
            f.write(f"@r{i}\n{seqs[s:e].tobytes().decode()}\n+\n{''.join(chr(33 + q) for q in quals[s:e])}\n")
    subprocess.check_call(GUARD + [cli, "index", "-g", fa])
    base = GUARD + [cli, "map", "-r", fq, "-g", fa, "-l", "single_stranded", "-p", "0.03", "-f", "0.5", "-t", "0.5", "-d", "0.02", "-s", "1.0", "-i", "0.001", "--seed", "7",
                    "--batch_size", "1000"]
    subprocess.check_call(base + ["-o", str(tmp_path / "plain.bam")])
    plain = _decoded(str(tmp_path / "plain.bam"))
    assert len(plain[2]) == n_reads == 4500
    idx = mapad_amd.Index.open(fa)
    params = mapad_amd.params_from_cli(library="single_stranded", five_prime_overhang=0.5, three_prime_overhang=0.5, ds_deamination_rate=0.02, ss_deamination_rate=1.0,
                                       poisson_prob=0.03, indel_rate=0.001)

    bound_cache = {}

    def binding_of(mode, flt, rule):
        """the binding's summary and consensus for the same reads and seed"""
        if (mode, flt, rule) not in bound_cache:
            ctx = mapad_amd.Context(idx, params, 0)
            try:
                ctx.set_pileup(mode, *flt)
                ctx.hits_to_records(ctx.map_batch(*batch), *batch, seed=7)
                bound_cache[(mode, flt, rule)] = (ctx.pileup(*rule), [ctx.pileup_consensus(t, 0, n, *rule) for t, n in enumerate(lengths)])
            finally:
                ctx.close()
        return bound_cache[(mode, flt, rule)]

    def check(name, extra, mode, flt, rule, tsv=True, fasta=True):
        bam, tsv_path, fa_path = str(tmp_path / f"{name}.bam"), str(tmp_path / f"{name}.tsv"), str(tmp_path / f"{name}.fa")
        cmd = base + ["-o", bam] + (["--pileup", tsv_path] if tsv else []) + (["--consensus", fa_path] if fasta else []) + extra
        pr = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True)
        assert "pileup (%s)" % ("unique" if mode == 2 else "all") in pr.stderr and "columns counted" in pr.stderr, pr.stderr
        assert _decoded(bam) == plain, name
        want = pu.from_bam(lengths, read_bam(bam)[2], mode, *flt)
        bound, bound_cons = binding_of(mode, flt, rule)
        pu.assert_equal(bound, want, *rule, what=name + ": the binding against the numpy table of the BAM")
        if tsv:
            head, scalars, rows = _read_tsv(tsv_path)
            assert head == {"mode": "unique" if mode == 2 else "all", "min_bq": str(flt[0]), "mask5": str(flt[1]), "mask3": str(flt[2]), "min_depth": str(rule[0]),
                            "min_percent": str(rule[1]), "contigs": "2"}
            assert all(scalars[k] == bound[k] == want[k] for k in pu.SCALARS) and scalars["reads_seen"] == n_reads and scalars["batches"] >= 1
            assert rows == bound["contigs"] and [r["name"] for r in rows] == ["chr1", "chr2"] == [r[0] for r in plain[1]]
        if fasta:
            records = _read_fasta(fa_path)
            assert [r[0] for r in records] == ["chr1", "chr2"]
            for t, (_, s) in enumerate(records):
                assert np.array_equal(s, bound_cons[t]) and np.array_equal(s, pu.consensus(want["counts"][t], *rule)), (name, t)
                assert (s == ord("N")).any() and (s != ord("N")).any()
        assert want["reads"] > 0 and want["insertions"] > 0 and want["deleted_columns"] > 0 and want["columns_not_acgt"] > 0
        return want

    all_run = check("all", [], 1, (0, 0, 0), (1, 0))
    assert all_run["columns_masked"] == 0 and all_run["columns_low_quality"] == 0
    flt = check("filtered_collapsed", ["--collapse_duplicates", "--pileup_min_bq", "30", "--pileup_mask5", "3", "--pileup_mask3", "2", "--consensus_min_depth", "2",
                                       "--consensus_min_percent", "70"], 1, (30, 3, 2), (2, 70))
    assert flt["columns_masked"] > 0 and flt["columns_low_quality"] > 0 and flt["reads"] == all_run["reads"]
    unique = check("unique_coalesced", ["--pileup_unique", "--coalesce", "2"], 2, (0, 0, 0), (1, 0), fasta=False)
    assert unique["reads"] < all_run["reads"]
    check("consensus_alone", [], 1, (0, 0, 0), (1, 0), tsv=False)  # --consensus alone implies mode 1
    assert open(str(tmp_path / "consensus_alone.fa")).read() == open(str(tmp_path / "all.fa")).read()
    # the pileup beside the coverage and the damage profile in one run: each file as in its own run
    bam, tsv, cov, dmg = (str(tmp_path / n) for n in ("both.bam", "both.tsv", "both_cov.tsv", "both_damage.tsv"))
    subprocess.check_call(base + ["-o", bam, "--pileup", tsv, "--coverage", cov, "--damage_profile", dmg])
    assert _decoded(bam) == plain and _read_tsv(tsv) == _read_tsv(str(tmp_path / "all.tsv"))
    for bad in (["--pileup_min_bq", "30"], ["--pileup", tsv, "--consensus_min_depth", "0"]):  # a filter without a pileup; a depth of 0: refused
        assert subprocess.run(base + ["-o", str(tmp_path / "bad.bam")] + bad, stderr=subprocess.DEVNULL).returncode != 0
