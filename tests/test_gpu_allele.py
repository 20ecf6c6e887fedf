"""The allele likelihoods on the GPU (run with -m gpu on an MI355X): what allele_kernel accumulates in a context while batches are converted to records, and
what allele_call_kernel makes of it, equals mapad_allele_host_* over the same fetched results, reads and seeds bit for bit — cells, depths, scalars, per-contig
statistics, consensus bytes and quality bytes — on reads chosen so that every branch of the kernel runs, under duplicate collapsing, with reads left out by
the duplicate marking and the damage score, across the pieces of a consensus window, after a merge of two contexts and through the CLI; and off is off.  A
reference of two contigs of a few kb and a few hundred reads: every test takes seconds."""
import re
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import build as mbuild
from mapad_amd import synth

import allele_util as au
import damage_util as du
import pileup_util as pu
from bam_util import read_bam
from kat_util import resolve_params
from parity_util import DAMAGE, IGNORE_BQ

pytestmark = pytest.mark.gpu

DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 99
GUARD = ["timeout", "-k", "10", "300"]  # every GPU child process under a time limit of its own
TOTAL, SPLIT = 9_000, 4_001
LENGTHS = [SPLIT, TOTAL - SPLIT]
RULES = [(1, 3.0), (2, 0.5)]            # (min_depth, min_margin in bits)
SETTINGS = [(1, (0, 0, 0)), (2, (25, 3, 2)), (1, (0, 12, 10))]  # (mode, (min_bq, mask5, mask3)); the last masks a read of 20 bases entirely
MODELS = {"ss": DAMAGE, "ignore_bq": IGNORE_BQ}  # 256 quality levels and one


@pytest.fixture(scope="module")
def world():
    g = synth.genome(TOTAL, seed=83)
    g[7_000:7_200] = g[2_000:2_200]  # a repeat: reads from it have X0 > 1 (mode 2 leaves them out)
    return g, mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])


def with_base(read, at, b):
    read = read.copy()
    read[at] = b
    return read


def hand_reads(g):
    """lengths 20, 63, 64, 65 and 130 on both strands, plain, with two reference bases deleted and with a base inserted (tracks of 63..132 operations: one, two
    and three trips of 64 lanes, the carry in use); reads with N on either strand; reads ending on a contig's last base and on the text's last base, on either
    strand; reads on the contigs' first bases"""
    other = lambda b: np.frombuffer(b"ACGT", np.uint8)[(int(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), b)) + 1) & 3]  # noqa: E731
    reads, at = [], 100
    for L in (20, 63, 64, 65, 130):
        for rev in (False, True):
            kinds = [g[at:at + L]]  # plain reads on c1, the others on c2 on either side of the repeat's copy
            if L > 20:
                half, d, i = L // 2, at + 4_100, at + 7_200
                kinds.append(np.concatenate([g[d:d + half], g[d + 2 + half:d + 2 + L]]))                       # two reference bases deleted
                kinds.append(np.concatenate([g[i:i + half], other(g[i + half])[None], g[i + half:i + L - 1]]))  # one base inserted
            reads += [synth.revcomp(r) if rev else r for r in kinds]
            at += 140
    reads += [with_base(g[1_500:1_550], 20, ord("N")), with_base(synth.revcomp(g[5_000:5_064]), 40, ord("N")), with_base(g[5_300:5_430], 100, ord("N"))]
    reads += [g[0:40], g[SPLIT:SPLIT + 40], g[SPLIT - 40:SPLIT], synth.revcomp(g[SPLIT - 63:SPLIT]), g[TOTAL - 40:TOTAL], synth.revcomp(g[TOTAL - 65:TOTAL])]
    return reads


def mixed_batch(g, n=300, seed=5):
    hand = pu.hand_made(hand_reads(g), qual=30)
    hq = hand[1].copy()
    hq[::7] = 24  # below a floor of 25
    hq[3::11] = 2
    return pu.concat(synth.reads(g, n, seed=seed, qual_range=(2, 40), damage=DMG, len_range=(20, 140), indel_frac=0.3),
                     synth.reads(g[2_000:2_200], n // 10, 45, seed=seed + 1, exo_frac=0.0, damage=DMG), (hand[0], hq, hand[2]))


def host_of(idx, params, res, batch, mode, flt=(0, 0, 0), seed=SEED, into=None, skip=None):
    return (into if into is not None else mb.AlleleHost(idx, mode, *flt)).add(params, res, *batch, seed=seed, skip=skip)


def assert_device_equals_host(ctx, acc, what=""):
    au.assert_same_accumulators(au.ContextView(ctx), acc, LENGTHS, RULES, what)
    return ctx.allele_summary(*RULES[0])


@pytest.mark.parametrize("model", list(MODELS))
def test_device_equals_the_host_path(world, model):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(MODELS[model]))
    batch = mixed_batch(g)
    n = len(batch[2]) - 1
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_allele_likelihoods(*((SETTINGS[0][0],) + SETTINGS[0][1]))
        res = ctx.map_batch(*batch)
        for mode, flt in SETTINGS:
            ctx.set_allele_likelihoods(mode, *flt)  # a change of any argument starts an empty table: the batch, still resident, counts into it
            recs = ctx.hits_to_records(res, *batch, seed=SEED)
            acc = host_of(idx, params, res, batch, mode, flt)
            got = assert_device_equals_host(ctx, acc, f"{model}, mode {mode}, filters {flt}")
            assert got["batches"] == 1 and got["reads_seen"] == n and 0 < got["reads"] < n and got["accumulate_ms"] > 0.0 and got["summary_ms"] > 0.0
            assert (got["mode"], got["min_base_quality"], got["mask5"], got["mask3"]) == (mode,) + flt and got["columns_counted"] > 0 and got["columns_not_acgt"] >= 3
            if flt == (0, 0, 0):  # and the table built in numpy from the device's records
                want = au.from_records(params, LENGTHS, recs, batch, mode)
                au.assert_equal(got, want, *RULES[0], what=model, cells_of=ctx.allele_cells, consensus_of=ctx.allele_consensus)
                assert got["columns_masked"] == 0 and got["columns_low_quality"] == 0
            else:
                assert got["columns_masked"] > 0 and (got["columns_low_quality"] > 0) == (flt[0] > 0)
        # the batch is what it is meant to be
        mapped = [r for r in recs if r["mapped"]]
        spans = [sum(int(k) for k, _ in pu._CIGAR.findall(r["cigar"])) for r in mapped]
        assert {r["reverse"] for r in mapped if "D" in r["cigar"]} == {False, True} and {r["reverse"] for r in mapped if "I" in r["cigar"]} == {False, True}
        assert {20, 63, 64, 65, 130} <= set(spans) and any(s in (66, 67) for s in spans) and max(spans) > 128
        ends = {(r["tid"], r["pos"] + sum(int(k) for k, o in pu._CIGAR.findall(r["cigar"]) if o != "I"), r["reverse"]) for r in mapped}
        assert {(0, SPLIT, False), (0, SPLIT, True), (1, LENGTHS[1], False), (1, LENGTHS[1], True)} <= ends
        assert any(r["xt"] != "U" for r in mapped)
    finally:
        ctx.close()


def test_a_batch_counts_once_collapsing_changes_nothing_and_reset_zeroes(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = du.with_duplicates(mixed_batch(g, seed=15), 200, seed=3)
    got = {}
    for collapse in (True, False):
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_collapse_duplicates(collapse)
            ctx.set_allele_likelihoods(1)
            res = ctx.map_batch(*batch)
            if collapse:
                info = ctx.collapse_info()
                assert info[1] < info[0] == len(batch[2]) - 1
            ctx.hits_to_records(res, *batch, seed=SEED)
            acc = host_of(idx, params, res, batch, 1)
            once = assert_device_equals_host(ctx, acc, f"collapse={collapse}")
            ctx.hits_to_records(res, *batch, seed=SEED)  # the same result again, then the same batch through mapad_records_device
            ctx.records_device(seed=SEED)
            again = assert_device_equals_host(ctx, acc, f"collapse={collapse}, converted three times")
            assert again["batches"] == once["batches"] == 1
            got[collapse] = [ctx.allele_cells(t, 0, n) for t, n in enumerate(LENGTHS)], {k: once[k] for k in pu.SCALARS}
            if not collapse:
                ctx.allele_reset()
                zero = ctx.allele_summary()
                assert zero["batches"] == 0 and zero["mode"] == 1 and all(zero[k] == 0 for k in pu.SCALARS) and zero["accumulate_ms"] == 0.0
                assert all(not ctx.allele_cells(t, 0, n)[0].any() and not ctx.allele_cells(t, 0, n)[1].any() for t, n in enumerate(LENGTHS))
                assert bytes(ctx.allele_consensus(0, 0, 5)[0]) == b"NNNNN"
                ctx.hits_to_records(res, *batch, seed=SEED)  # nothing has been counted: the batch, still resident, counts into the fresh table
                assert_device_equals_host(ctx, acc, "after the reset")
        finally:
            ctx.close()
    assert got[True][1] == got[False][1]
    for (al, ad), (bl, bd) in zip(got[True][0], got[False][0]):
        assert np.array_equal(al, bl) and np.array_equal(ad, bd)


@pytest.mark.parametrize("how", ["mark_duplicates", "damage_score"])
def test_reads_left_out_by_mode_2_are_absent(world, how):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = du.with_duplicates(mixed_batch(g, seed=25), 150, seed=9)
    n = len(batch[2]) - 1
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_allele_likelihoods(1, 25, 2, 2)
        if how == "mark_duplicates":
            ctx.set_mark_duplicates(2)
            res = ctx.map_batch(*batch)
            recs = ctx.hits_to_records(res, *batch, seed=SEED, as_arrays=True)[0]
            skip = ((recs["flags"] & 0x400) != 0).astype(np.uint8)
        else:
            hq, hs, _ = mb.damage_score_host(idx, params, ctx.map_batch(*batch), *batch, seed=SEED)
            thr_q = int(np.sort(hq[hs == 1])[int(hs.sum()) // 2])  # a threshold that splits the batch
            ctx.set_damage_score(2, thr_q / 256.0)
            res = ctx.map_batch(*batch)
            _, _, score_q, scored = ctx.hits_to_records(res, *batch, seed=SEED, as_arrays=True)
            skip = ((scored == 1) & (score_q < thr_q)).astype(np.uint8)
        assert 0 < int(skip.sum()) < n
        got = assert_device_equals_host(ctx, host_of(idx, params, res, batch, 1, (25, 2, 2), skip=skip), how)
        everyone = host_of(idx, params, res, batch, 1, (25, 2, 2)).summary()
        assert got["reads_seen"] == n == everyone["reads_seen"] and got["reads"] < everyone["reads"] and got["columns_counted"] < everyone["columns_counted"]
    finally:
        ctx.close()


def test_a_window_across_the_pieces_of_a_consensus_and_two_contexts_merged(world, monkeypatch):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    first, second = mixed_batch(g, seed=35), mixed_batch(g, 200, seed=45)
    n_first = len(first[2]) - 1
    seed2 = int(mapad_amd.lib().mapad_records_seed_at(SEED, n_first))
    one, a, b = (mapad_amd.Context(idx, params, 0) for _ in range(3))
    try:
        for c in (one, a, b):
            c.set_allele_likelihoods(1, 10, 1, 1)
        acc = None
        for c, batch, seed in ((one, first, SEED), (one, second, seed2), (a, first, SEED), (b, second, seed2)):
            res = c.map_batch(*batch)
            c.hits_to_records(res, *batch, seed=seed)
            if c is one:
                acc = host_of(idx, params, res, batch, 1, (10, 1, 1), seed=seed, into=acc)
        whole = assert_device_equals_host(one, acc, "two batches")
        # a window that spans piece boundaries gives the bytes of the whole-contig call
        full = [one.allele_consensus(t, 0, n, 1, 3.0) for t, n in enumerate(LENGTHS)]
        monkeypatch.setenv("MAPAD_ALLELE_PIECE", "1000")  # read at every call
        for t, n in enumerate(LENGTHS):
            bases, quals = one.allele_consensus(t, 0, n, 1, 3.0)  # five pieces, the last one short
            assert np.array_equal(bases, full[t][0]) and np.array_equal(quals, full[t][1]), t
            bases, quals = one.allele_consensus(t, 937, 2_101, 1, 3.0)
            assert np.array_equal(bases, full[t][0][937:937 + 2_101]) and np.array_equal(quals, full[t][1][937:937 + 2_101]), t
        monkeypatch.setenv("MAPAD_ALLELE_PIECE", "1")
        bases, quals = one.allele_consensus(0, 100, 70, 1, 3.0)
        assert np.array_equal(bases, full[0][0][100:170]) and np.array_equal(quals, full[0][1][100:170]) and (bases != ord("N")).any() and quals.any()
        monkeypatch.delenv("MAPAD_ALLELE_PIECE")
        # two contexts that took one batch each, merged: the context that took both
        half = a.allele_summary()
        assert half["batches"] == 1 and half["reads"] < whole["reads"]
        a.allele_merge(b)
        merged = assert_device_equals_host(a, acc, "merged")
        au.assert_equal(merged, whole, *RULES[0], what="merged against the one context")
        assert merged["batches"] == 2 and b.allele_summary()["batches"] == 1  # the source keeps its own
        for other in ((1, 10, 1, 2), (1, 9, 1, 1), (2, 10, 1, 1), (0, 0, 0, 0)):  # another filter, another mode, off: not the same table
            b.set_allele_likelihoods(*other)
            with pytest.raises(mapad_amd.MapadError) as e:
                a.allele_merge(b)
            assert e.value.code == -1  # MAPAD_ERR_INVALID
        with pytest.raises(mapad_amd.MapadError) as e:
            a.allele_merge(a)
        assert e.value.code == -1
        au.assert_equal(a.allele_summary(), whole, *RULES[0], what="after the refused merges")
    finally:
        for c in (one, a, b):
            c.close()


def _record_texts(recs, text):
    """the CIGAR, MD and XA bytes of every record, in record order"""
    blob = text.tobytes()
    return [tuple(blob[int(r[k + "_off"]):int(r[k + "_off"]) + int(r[k + "_len"])] for k in ("cigar", "md", "xa")) for r in recs]


def _assert_same_records(a, b, same_pool):
    """every field of every record and the CIGAR, MD and XA bytes its offsets point to.  Pool offsets only on the host text path (same_pool): the device text
    pool is filled in arrival order (tests/test_gpu_dedup.py explains the comparison)."""
    assert len(a) == len(b) == 2 and len(a[0]) == len(b[0]) and _record_texts(a[0], a[1]) == _record_texts(b[0], b[1])
    for k in a[0].dtype.names:
        if k and not k.startswith("_") and (same_pool or not k.endswith("_off")):
            assert np.array_equal(a[0][k], b[0][k]), k
    if same_pool:
        assert a[1].tobytes() == b[1].tobytes()


def _error_of(call):
    try:
        call()
    except mapad_amd.MapadError as e:
        return e.code
    return None


def test_off_is_off_and_uploaded_hits_are_refused_only_while_on(world, monkeypatch):
    """With mode 0 — never switched on, and switched off again — results and records are what they are without the feature, field by field and by the CIGAR / MD /
    XA bytes their offsets point to, on both records paths, and every read-out answers as an empty table does.  (The library keeps no allocation accounting that a
    test could ask; that mode 0 frees the arrays is in mapad_ctx_set_allele_likelihoods, and nothing is allocated before the switch-on.)"""
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, seed=65)
    fresh, a, b = (mapad_amd.Context(idx, params, 0) for _ in range(3))

    def both_paths(ctx, res):
        out = {"device": ctx.hits_to_records(res, *batch, seed=SEED, as_arrays=True)}
        with monkeypatch.context() as m:
            m.setenv("MAPAD_RECORDS_TEXT", "host")  # read at every records call
            out["host"] = ctx.hits_to_records(res, *batch, seed=SEED, as_arrays=True)
        return out

    try:
        res_plain = fresh.map_batch(*batch)
        want = both_paths(fresh, res_plain)
        never = fresh.allele_summary()
        assert never["mode"] == 0 and never["batches"] == 0 and all(never[k] == 0 for k in pu.SCALARS) and [c["length"] for c in never["contigs"]] == LENGTHS
        assert all(c["sites_covered"] == 0 and c["sites_called"] == 0 and c["max_depth"] == 0 and c["margin_sum_q"] == 0 for c in never["contigs"])
        ll, depth = fresh.allele_cells(0, 100, 1000)
        assert not ll.any() and not depth.any() and bytes(fresh.allele_consensus(1, 0, 4)[0]) == b"NNNN" and not fresh.allele_consensus(1, 0, 4)[1].any()
        a.set_allele_likelihoods(2, 20, 1, 1)
        res_on = a.map_batch(*batch)
        on = both_paths(a, res_on)
        assert np.array_equal(res_on.hit_begin, res_plain.hit_begin) and np.array_equal(res_on.ops, res_plain.ops)
        assert all(res_on.hits_arr[k].tobytes() == res_plain.hits_arr[k].tobytes() for k in ("lower", "lower_rev", "size", "score", "n_ops", "ops_offset"))
        _assert_same_records(on["device"], want["device"], same_pool=False)  # the sums change no record
        _assert_same_records(on["host"], want["host"], same_pool=True)
        assert a.allele_summary()["batches"] == 1
        a.set_allele_likelihoods(0)
        off = both_paths(a, a.map_batch(*batch))
        _assert_same_records(off["device"], want["device"], same_pool=False)
        _assert_same_records(off["host"], want["host"], same_pool=True)
        gone = a.allele_summary()
        assert gone["mode"] == 0 and gone["batches"] == 0 and gone["reads_seen"] == 0 and not a.allele_cells(0, 0, LENGTHS[0])[1].any()
        # another context's result: its hits are uploaded, its reads are not on the device
        plain = fresh.hits_to_records(res_on, *batch, seed=SEED)
        assert b.hits_to_records(res_on, *batch, seed=SEED) == plain
        b.set_allele_likelihoods(1)
        with pytest.raises(mapad_amd.MapadError) as e:
            b.hits_to_records(res_on, *batch, seed=SEED)
        assert e.value.code == -9  # MAPAD_ERR_UNSUPPORTED
        assert b.allele_summary()["batches"] == 0
        b.set_allele_likelihoods(0)
        assert b.hits_to_records(res_on, *batch, seed=SEED) == plain
        nan = float("nan")
        for bad in (lambda: a.set_allele_likelihoods(3), lambda: a.set_allele_likelihoods(-1), lambda: a.set_allele_likelihoods(1, 256), lambda: a.set_allele_likelihoods(1, 0, 65536),
                    lambda: a.set_allele_likelihoods(1, 0, 0, 65536), lambda: a.allele_summary(0, 3.0), lambda: a.allele_summary(1, nan), lambda: a.allele_consensus(0, 0, 4, 0, 3.0),
                    lambda: a.allele_consensus(0, 0, 4, 1, nan), lambda: a.allele_cells(0, LENGTHS[0] - 3, 4), lambda: a.allele_cells(2, 0, 1)):
            assert _error_of(bad) == -1  # MAPAD_ERR_INVALID
        monkeypatch.setenv("MAPAD_ALLELE_LIK", "2")  # the default of new contexts
        c = mapad_amd.Context(idx, params, 0)
        try:
            assert c.allele_summary()["mode"] == 2
        finally:
            c.close()
    finally:
        for c in (fresh, a, b):
            c.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def _decoded(path):
    text, refs, recs = read_bam(path)
    out = []
    for r in recs:
        tags = {k: v for k, v in r["tags"].items() if k != "XD"}  # (XD: wall time per read)
        out.append((r["name"], r["flags"], r["tid"], r["pos"], r["mapq"], r["bin"], r["cigar"], r["seq"], r["qual"], tuple(sorted(tags.items())), tuple(r["tag_order"])))
    return re.sub(r"\tCL:[^\t\n]*", "", text), refs, out  # (CL: the command line, which names the options and the output files)


def _read_tsv(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("#mapad-amd-allele-likelihoods v1 ")
    head = dict(kv.split("=") for kv in lines[0].split()[2:])
    assert list(head) == ["mode", "min_bq", "mask5", "mask3", "min_depth", "min_margin_q", "contigs"]
    names = lines[1][1:].split("\t")
    assert names == list(pu.SCALARS) + ["batches"] and lines[1][0] == "#"
    scalars = dict(zip(names, (int(x) for x in lines[2].split("\t"))))
    assert lines[3] == "#rname\tlength\tsites_covered\tsites_deep\tsites_called\tcalled_A\tcalled_C\tcalled_G\tcalled_T\tmaxdepth\tmargin_sum_q"
    rows = []
    for ln in lines[4:]:
        f = ln.split("\t")
        assert len(f) == 11
        v = [int(x) for x in f[1:]]
        rows.append({"name": f[0], "length": v[0], "sites_covered": v[1], "sites_deep": v[2], "sites_called": v[3], "called": v[4:8], "max_depth": v[8], "margin_sum_q": v[9]})
    assert len(rows) == int(head["contigs"])
    return head, scalars, rows


def _read_fasta(path):
    out = []
    for block in open(path).read().split(">")[1:]:
        lines = block.splitlines()
        assert all(len(ln) == 60 for ln in lines[1:-1]) and 0 < len(lines[-1]) <= 60
        out.append((lines[0], np.frombuffer("".join(lines[1:]).encode(), np.uint8)))
    return out


def test_cli_writes_the_summary_the_consensus_and_its_qualities(tmp_path):
    """The BAM of a run with --allele_likelihoods / --damage_consensus holds the same records as one without (all but the XD tag, wall time, and the header's CL
    field, the command line itself); the TSV, the FASTA and the quality file equal what the binding gives for the same reads, parameters and seed."""
    mapad_amd.lib()
    cli = mbuild.build_cli()
    g = synth.genome(TOTAL, seed=17)
    fa, fq = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fastq")
    with open(fa, "w") as f:
        for name, s in (("chr1", g[:SPLIT].tobytes().decode()), ("chr2", g[SPLIT:].tobytes().decode())):
            f.write(f">{name}\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    batch = pu.concat(synth.reads(g, 600, seed=23, qual_range=(2, 40), damage=DMG, len_range=(25, 110), indel_frac=0.3),
                      pu.hand_made([g[0:40], g[SPLIT - 40:SPLIT], g[TOTAL - 40:TOTAL], with_base(g[5_000:5_060], 30, ord("N"))], qual=31))
    seqs, quals, offsets = batch
    n_reads = len(offsets) - 1
    with open(fq, "w") as f:
        for i in range(n_reads):
            s, e = int(offsets[i]), int(offsets[i + 1])
            f.write(f"@r{i}\n{seqs[s:e].tobytes().decode()}\n+\n{''.join(chr(33 + q) for q in quals[s:e])}\n")
    subprocess.check_call(GUARD + [cli, "index", "-g", fa])
    base = GUARD + [cli, "map", "-r", fq, "-g", fa, "-l", "single_stranded", "-p", "0.03", "-f", "0.5", "-t", "0.5", "-d", "0.02", "-s", "1.0", "-i", "0.001", "--seed", "7",
                    "--batch_size", "250"]
    subprocess.check_call(base + ["-o", str(tmp_path / "plain.bam")])
    plain = _decoded(str(tmp_path / "plain.bam"))
    assert len(plain[2]) == n_reads
    idx = mapad_amd.Index.open(fa)
    params = mapad_amd.params_from_cli(library="single_stranded", five_prime_overhang=0.5, three_prime_overhang=0.5, ds_deamination_rate=0.02, ss_deamination_rate=1.0,
                                       poisson_prob=0.03, indel_rate=0.001)
    for name, extra, mode, flt, rule in (("all", [], 1, (0, 0, 0), (1, 3.0)),
                                         ("unique_filtered", ["--allele_unique", "--allele_min_bq", "20", "--allele_mask5", "2", "--allele_mask3", "1", "--damage_consensus_min_depth", "2",
                                                              "--damage_consensus_min_margin", "6.5"], 2, (20, 2, 1), (2, 6.5))):
        bam, tsv, cons, qual = (str(tmp_path / f"{name}.{ext}") for ext in ("bam", "tsv", "fa", "qual"))
        pr = subprocess.run(base + ["-o", bam, "--allele_likelihoods", tsv, "--damage_consensus", cons, "--damage_consensus_qual", qual] + extra, check=True, stderr=subprocess.PIPE,
                            text=True)
        assert "allele likelihoods (%s)" % ("unique" if mode == 2 else "all") in pr.stderr and "columns counted" in pr.stderr, pr.stderr
        assert _decoded(bam) == plain, name
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_allele_likelihoods(mode, *flt)
            ctx.hits_to_records(ctx.map_batch(*batch), *batch, seed=7)
            bound, bound_cons = ctx.allele_summary(*rule), [ctx.allele_consensus(t, 0, n, *rule) for t, n in enumerate(LENGTHS)]
        finally:
            ctx.close()
        head, scalars, rows = _read_tsv(tsv)
        assert head == {"mode": "unique" if mode == 2 else "all", "min_bq": str(flt[0]), "mask5": str(flt[1]), "mask3": str(flt[2]), "min_depth": str(rule[0]),
                        "min_margin_q": str(au.min_margin_q(rule[1])), "contigs": "2"}
        assert all(scalars[k] == bound[k] for k in pu.SCALARS) and scalars["reads_seen"] == n_reads and scalars["batches"] == 3 and scalars["reads"] > 0
        assert rows == [{k: c[k] for k in ("name",) + au.CONTIG_KEYS} for c in bound["contigs"]] and [r["name"] for r in rows] == ["chr1", "chr2"]
        records = _read_fasta(cons)
        qlines = open(qual).read().split("\n")
        assert [r[0] for r in records] == ["chr1", "chr2"] and len(qlines) == 3 and qlines[2] == ""
        for t, (_, s) in enumerate(records):
            assert np.array_equal(s, bound_cons[t][0]) and (s == ord("N")).any() and (s != ord("N")).any(), (name, t)
            assert np.array_equal(np.frombuffer(qlines[t].encode(), np.uint8), 33 + np.minimum(bound_cons[t][1], 93)), (name, t)
    # the options need their switch
    for bad in (["--allele_unique"], ["--allele_min_bq", "3"], ["--damage_consensus_qual", str(tmp_path / "q")], ["--damage_consensus_min_margin", "2"]):
        assert subprocess.run(base + ["-o", str(tmp_path / "bad.bam")] + bad, stderr=subprocess.PIPE).returncode != 0
