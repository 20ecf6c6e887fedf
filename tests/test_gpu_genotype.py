"""The diploid genotype likelihoods on the GPU (run with -m gpu on an MI355X): what genotype_kernel accumulates behind allele_kernel while batches are
converted to records, and what genotype_call_kernel makes of it, equals the host path (mapad_allele_host_* with genotypes on) over the same fetched results,
reads and seeds bit for bit — het cells, genotype bytes, GQ bytes and every summary word — on reads chosen so that every branch of the kernel runs, with reads
from a second haplotype so that het genotypes lead somewhere; under duplicate collapsing, with reads left out by the duplicate marking and the damage score,
across the pieces of a window, after a merge of two contexts and through the CLI's TSV and VCF; and off is off.  A reference of two contigs of a few kb and a
few hundred reads: every test takes seconds."""
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
import genotype_util as gu
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
RULES = [(1, 3.0, 0.0), (2, 0.5, 10.0)]  # (min_depth, min_margin in bits, het penalty in bits)
ARULES = [(1, 3.0), (2, 0.5)]
SETTINGS = [(1, (0, 0, 0)), (2, (25, 3, 2)), (1, (0, 12, 10))]  # (mode, (min_bq, mask5, mask3)); the last masks a read of 20 bases entirely
MODELS = {"ss": DAMAGE, "ignore_bq": IGNORE_BQ}  # 256 quality levels and one
ACGT = np.frombuffer(b"ACGT", np.uint8)


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
    other = lambda b: ACGT[(int(np.searchsorted(ACGT, b)) + 1) & 3]  # noqa: E731
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
    """the hand-made reads, n synthetic reads with indels and qualities 2..40, reads from the repeat, and n / 2 reads from a second haplotype (a SNP every 50
    bases): het genotypes where both haplotypes are covered, hom-alt ones where only the second is"""
    hand = pu.hand_made(hand_reads(g), qual=30)
    hq = hand[1].copy()
    hq[::7] = 24  # below a floor of 25
    hq[3::11] = 2
    hap, _ = gu.second_haplotype(g, 50, seed=seed + 2)
    return pu.concat(synth.reads(g, n, seed=seed, qual_range=(2, 40), damage=DMG, len_range=(20, 140), indel_frac=0.3),
                     synth.reads(g[2_000:2_200], n // 10, 45, seed=seed + 1, exo_frac=0.0, damage=DMG),
                     synth.reads(hap, n // 2, 70, seed=seed + 3, exo_frac=0.0, qual_range=(20, 40), damage=DMG), (hand[0], hq, hand[2]))


def host_of(idx, params, res, batch, mode, flt=(0, 0, 0), seed=SEED, into=None, skip=None):
    return (into if into is not None else mb.AlleleHost(idx, mode, *flt, genotypes=True)).add(params, res, *batch, seed=seed, skip=skip)


def assert_device_equals_host(ctx, acc, what=""):
    gu.assert_same(ctx, acc, LENGTHS, RULES, what)
    au.assert_same_accumulators(au.ContextView(ctx), acc, LENGTHS, ARULES, what)  # and what it rides on
    return ctx.genotype_summary(*RULES[0])


def on(ctx, mode=1, flt=(0, 0, 0)):
    ctx.set_allele_likelihoods(mode, *flt)
    ctx.set_genotype_likelihoods(True)


def _error_of(call):
    try:
        call()
    except mapad_amd.MapadError as e:
        return e.code
    return None


@pytest.mark.parametrize("model", list(MODELS))
def test_device_equals_the_host_path(world, model):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(MODELS[model]))
    batch = mixed_batch(g)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        on(ctx, *SETTINGS[0])
        res = ctx.map_batch(*batch)
        for mode, flt in SETTINGS:
            ctx.set_allele_likelihoods(mode, *flt)  # a change of any allele argument empties both tables: the batch, still resident, counts into them
            assert ctx.genotype_summary()["on"] == 1
            recs = ctx.hits_to_records(res, *batch, seed=SEED)
            acc = host_of(idx, params, res, batch, mode, flt)
            got = assert_device_equals_host(ctx, acc, f"{model}, mode {mode}, filters {flt}")
            assert got["batches"] == 1 and got["accumulate_ms"] > 0.0 and got["summary_ms"] > 0.0 and ctx.allele_summary()["batches"] == 1
            if flt == (0, 0, 0):  # and the table built in numpy from the device's records
                want = gu.from_records(params, LENGTHS, recs, batch, mode)
                for rule in RULES:
                    gu.assert_equal(ctx, want, rule, what=f"{model}, rule {rule}")
                # het genotypes and hom-alt genotypes both lead somewhere
                code = np.searchsorted(ACGT, g)
                calls, strict = (np.concatenate([ctx.genotype_calls(t, 0, n, *rule)[0] for t, n in enumerate(LENGTHS)]) for rule in RULES)
                assert ((calls >= 4) & (calls != gu.NO_CALL)).sum() >= 1 and ((calls < 4) & (calls == code)).sum() > 1000
                assert ((strict < 4) & (strict != code)).sum() >= 1  # (under the 10-bit penalty: a site only the second haplotype's reads cover)
                assert sum(sum(c["called"][4:]) for c in got["contigs"]) >= 1
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
            on(ctx)
            res = ctx.map_batch(*batch)
            ctx.hits_to_records(res, *batch, seed=SEED)
            acc = host_of(idx, params, res, batch, 1)
            once = assert_device_equals_host(ctx, acc, f"collapse={collapse}")
            ctx.hits_to_records(res, *batch, seed=SEED)  # the same result again, then the same batch through mapad_records_device
            ctx.records_device(seed=SEED)
            again = assert_device_equals_host(ctx, acc, f"collapse={collapse}, converted three times")
            assert again["batches"] == once["batches"] == 1
            got[collapse] = [ctx.genotype_cells(t, 0, n) for t, n in enumerate(LENGTHS)]
            assert any(h.any() for h in got[collapse])
            if not collapse:
                ctx.allele_reset()
                zero = ctx.genotype_summary()
                assert zero["on"] == 1 and zero["batches"] == 0 and zero["accumulate_ms"] == 0.0 and all(c["sites_covered"] == 0 for c in zero["contigs"])
                assert all(not ctx.genotype_cells(t, 0, n).any() for t, n in enumerate(LENGTHS)) and (ctx.genotype_calls(0, 0, 5)[0] == gu.NO_CALL).all()
                ctx.hits_to_records(res, *batch, seed=SEED)  # nothing has been counted: the batch, still resident, counts into the fresh table
                assert_device_equals_host(ctx, acc, "after the reset")
        finally:
            ctx.close()
    for a, b in zip(got[True], got[False]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("how", ["mark_duplicates", "damage_score"])
def test_reads_left_out_by_mode_2_are_absent(world, how):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = du.with_duplicates(mixed_batch(g, seed=25), 150, seed=9)
    n = len(batch[2]) - 1
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        on(ctx, 1, (25, 2, 2))
        if how == "mark_duplicates":
            ctx.set_mark_duplicates(2)
            res = ctx.map_batch(*batch)
            recs = ctx.hits_to_records(res, *batch, seed=SEED, as_arrays=True)[0]
            skip = ((recs["flags"] & 0x400) != 0).astype(np.uint8)
        else:
            hq, hs, _ = mb.damage_score_host(idx, params, ctx.map_batch(*batch), *batch, seed=SEED)
            thr_q = int(np.sort(hq[hs == 1])[int(hs.sum()) // 2])  # a threshold that splits the batch
            ctx.set_damage_score(2, thr_q / 256.0)
            ctx.allele_reset()  # (the batch mapped for the threshold was not converted; start clean all the same)
            res = ctx.map_batch(*batch)
            _, _, score_q, scored = ctx.hits_to_records(res, *batch, seed=SEED, as_arrays=True)
            skip = ((scored == 1) & (score_q < thr_q)).astype(np.uint8)
        assert 0 < int(skip.sum()) < n
        assert_device_equals_host(ctx, host_of(idx, params, res, batch, 1, (25, 2, 2), skip=skip), how)
        everyone = host_of(idx, params, res, batch, 1, (25, 2, 2))
        assert any(not np.array_equal(ctx.genotype_cells(t, 0, m), everyone.genotype_cells(t, 0, m)) for t, m in enumerate(LENGTHS))
    finally:
        ctx.close()


def test_a_window_across_the_pieces_and_two_contexts_merged(world, monkeypatch):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    first, second = mixed_batch(g, seed=35), mixed_batch(g, 200, seed=45)
    n_first = len(first[2]) - 1
    seed2 = int(mapad_amd.lib().mapad_records_seed_at(SEED, n_first))
    one, a, b = (mapad_amd.Context(idx, params, 0) for _ in range(3))
    rule = RULES[1]
    try:
        for c in (one, a, b):
            on(c, 1, (10, 1, 1))
        acc = None
        for c, batch, seed in ((one, first, SEED), (one, second, seed2), (a, first, SEED), (b, second, seed2)):
            res = c.map_batch(*batch)
            c.hits_to_records(res, *batch, seed=seed)
            if c is one:
                acc = host_of(idx, params, res, batch, 1, (10, 1, 1), seed=seed, into=acc)
        whole = assert_device_equals_host(one, acc, "two batches")
        # a window that spans piece boundaries gives the bytes of the whole-contig call
        full = [one.genotype_calls(t, 0, n, *rule) for t, n in enumerate(LENGTHS)]
        monkeypatch.setenv("MAPAD_ALLELE_PIECE", "1000")  # read at every call
        for t, n in enumerate(LENGTHS):
            gt, gq = one.genotype_calls(t, 0, n, *rule)  # five pieces, the last one short
            assert np.array_equal(gt, full[t][0]) and np.array_equal(gq, full[t][1]), t
            gt, gq = one.genotype_calls(t, 937, 2_101, *rule)
            assert np.array_equal(gt, full[t][0][937:937 + 2_101]) and np.array_equal(gq, full[t][1][937:937 + 2_101]), t
        monkeypatch.setenv("MAPAD_ALLELE_PIECE", "1")
        gt, gq = one.genotype_calls(0, 100, 70, *rule)
        assert np.array_equal(gt, full[0][0][100:170]) and np.array_equal(gq, full[0][1][100:170]) and (gt != gu.NO_CALL).any() and gq.any()
        monkeypatch.delenv("MAPAD_ALLELE_PIECE")
        # two contexts that took one batch each, merged: the context that took both
        assert a.genotype_summary()["batches"] == 1
        a.allele_merge(b)
        a.genotype_merge(b)
        merged = assert_device_equals_host(a, acc, "merged")
        assert merged["batches"] == 2 == whole["batches"] and b.genotype_summary()["batches"] == 1  # the source keeps its own
        gu.assert_same(a, one, LENGTHS, RULES, "merged against the one context")
        before = [a.genotype_cells(t, 0, n) for t, n in enumerate(LENGTHS)]
        b.set_genotype_likelihoods(False)  # off in the source
        assert _error_of(lambda: a.genotype_merge(b)) == -1  # MAPAD_ERR_INVALID
        for other in ((1, 10, 1, 2), (2, 10, 1, 1)):  # other allele settings
            b.set_allele_likelihoods(*other)
            b.set_genotype_likelihoods(True)
            assert _error_of(lambda: a.genotype_merge(b)) == -1
        assert _error_of(lambda: a.genotype_merge(a)) == -1
        assert all(np.array_equal(a.genotype_cells(t, 0, n), before[t]) for t, n in enumerate(LENGTHS))
        gu.assert_same(a, one, LENGTHS, RULES, "after the refused merges")
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


def test_off_is_off_and_the_switch_follows_the_allele_mode(world, monkeypatch):
    """With the feature never on, and switched off again, results and records are what they are without it on both records paths, and every read-out answers as
    an empty table does; with it on, the allele read-outs are what they are with it off."""
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
        never = fresh.genotype_summary()
        assert never["on"] == 0 and never["batches"] == 0 and [c["length"] for c in never["contigs"]] == LENGTHS
        assert all(c["sites_covered"] == 0 and c["sites_called"] == 0 and c["max_depth"] == 0 and c["margin_sum_q"] == 0 for c in never["contigs"])
        assert not fresh.genotype_cells(0, 100, 1000).any() and (fresh.genotype_calls(1, 0, 4)[0] == gu.NO_CALL).all() and not fresh.genotype_calls(1, 0, 4)[1].any()
        assert _error_of(lambda: fresh.set_genotype_likelihoods(True)) == -1  # not without an allele mode
        fresh.set_genotype_likelihoods(False)
        # allele likelihoods alone, then with the genotypes on top: the allele read-outs do not change, nor do the records
        a.set_allele_likelihoods(2, 20, 1, 1)
        res_a = a.map_batch(*batch)
        a.hits_to_records(res_a, *batch, seed=SEED)
        assert a.allele_summary()["batches"] == 1 and a.genotype_summary()["on"] == 0 and not a.genotype_cells(0, 0, LENGTHS[0]).any()
        a.set_genotype_likelihoods(True)  # switching on after a batch has been counted empties both tables
        assert a.allele_summary()["batches"] == 0 and not a.allele_cells(0, 0, LENGTHS[0])[1].any() and not a.genotype_cells(0, 0, LENGTHS[0]).any()
        both = both_paths(a, res_a)  # the batch, still resident, counts into both
        _assert_same_records(both["device"], want["device"], same_pool=False)
        _assert_same_records(both["host"], want["host"], same_pool=True)
        plain_acc = mb.AlleleHost(idx, 2, 20, 1, 1).add(params, res_a, *batch, seed=SEED)
        au.assert_same_accumulators(au.ContextView(a), plain_acc, LENGTHS, ARULES, "the allele read-outs with the genotypes on")
        assert a.genotype_summary()["batches"] == 1 and a.genotype_cells(0, 0, LENGTHS[0]).any()
        a.set_genotype_likelihoods(False)  # off again: both tables start empty, the allele likelihoods go on
        assert a.genotype_summary()["on"] == 0 and a.allele_summary()["batches"] == 0 and a.allele_summary()["mode"] == 2
        off = both_paths(a, a.map_batch(*batch))
        _assert_same_records(off["device"], want["device"], same_pool=False)
        _assert_same_records(off["host"], want["host"], same_pool=True)
        au.assert_same_accumulators(au.ContextView(a), plain_acc, LENGTHS, ARULES, "the allele read-outs with the genotypes off again")
        assert not a.genotype_cells(0, 0, LENGTHS[0]).any()
        a.set_genotype_likelihoods(True)
        a.set_allele_likelihoods(0)  # allele mode 0 switches the feature off
        assert a.genotype_summary()["on"] == 0 and _error_of(lambda: a.set_genotype_likelihoods(True)) == -1
        gone = both_paths(a, a.map_batch(*batch))
        _assert_same_records(gone["device"], want["device"], same_pool=False)
        _assert_same_records(gone["host"], want["host"], same_pool=True)
        # another context's result: its hits are uploaded, its reads are not on the device
        plain = fresh.hits_to_records(res_a, *batch, seed=SEED)
        assert b.hits_to_records(res_a, *batch, seed=SEED) == plain
        on(b)
        assert _error_of(lambda: b.hits_to_records(res_a, *batch, seed=SEED)) == -9  # MAPAD_ERR_UNSUPPORTED
        assert b.genotype_summary()["batches"] == 0
        b.set_allele_likelihoods(0)
        assert b.hits_to_records(res_a, *batch, seed=SEED) == plain
        on(b)
        nan = float("nan")
        for bad in (lambda: b.genotype_summary(0, 3.0, 0.0), lambda: b.genotype_summary(1, nan, 0.0), lambda: b.genotype_summary(1, 3.0, nan), lambda: b.genotype_summary(1, 3.0, -0.01),
                    lambda: b.genotype_calls(0, 0, 4, 0, 3.0, 0.0), lambda: b.genotype_calls(0, 0, 4, 1, 3.0, nan), lambda: b.genotype_calls(0, 0, 4, 1, 3.0, -1.0),
                    lambda: b.genotype_calls(0, LENGTHS[0] - 3, 4), lambda: b.genotype_cells(0, LENGTHS[0] - 3, 4), lambda: b.genotype_cells(2, 0, 1), lambda: b.genotype_calls(2, 0, 1)):
            assert _error_of(bad) == -1  # MAPAD_ERR_INVALID
        for env, want_on in (({"MAPAD_ALLELE_LIK": "1", "MAPAD_GENOTYPE_LIK": "1"}, 1), ({"MAPAD_GENOTYPE_LIK": "1"}, 0), ({"MAPAD_ALLELE_LIK": "1"}, 0)):  # the default of new contexts
            with monkeypatch.context() as m:
                for k, v in env.items():
                    m.setenv(k, v)
                c = mapad_amd.Context(idx, params, 0)
                try:
                    assert c.genotype_summary()["on"] == want_on and c.allele_summary()["mode"] == (1 if "MAPAD_ALLELE_LIK" in env else 0)
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
    assert lines[0].startswith("#mapad-amd-genotype-likelihoods v1 ")
    head = dict(kv.split("=") for kv in lines[0].split()[2:])
    assert list(head) == ["mode", "min_bq", "mask5", "mask3", "min_depth", "min_margin_q", "het_penalty_q", "contigs"]
    names = lines[1][1:].split("\t")
    assert names == list(pu.SCALARS) + ["batches"] and lines[1][0] == "#"
    scalars = dict(zip(names, (int(x) for x in lines[2].split("\t"))))
    assert lines[3] == "#rname\tlength\tsites_covered\tsites_deep\tsites_called\t" + "\t".join("called_" + x for x in gu.GENOTYPES) + "\tmaxdepth\tmargin_sum_q"
    rows = []
    for ln in lines[4:]:
        f = ln.split("\t")
        assert len(f) == 17
        v = [int(x) for x in f[1:]]
        rows.append({"name": f[0], "length": v[0], "sites_covered": v[1], "sites_deep": v[2], "sites_called": v[3], "called": v[4:14], "max_depth": v[14], "margin_sum_q": v[15]})
    assert len(rows) == int(head["contigs"])
    return head, scalars, rows


def _expected_vcf(names, ref, ll, het, depth, rule):
    """the VCF's data lines from cells and calls: one per called site whose genotype is not homozygous for an A/C/G/T REF"""
    out = []
    for t, name in enumerate(names):
        call, _, gq, _ = gu.calls(ll[t], het[t], depth[t], rule[0], au.min_margin_q(rule[1]), gu.penalty_q(rule[2]))
        g = gu.values(ll[t], het[t], gu.penalty_q(rule[2]))
        for i in np.flatnonzero(call != gu.NO_CALL):
            r = "ACGT".find(chr(ref[t][i]).upper())
            if r < 0 or call[i] == r:
                continue
            x, y = gu.ALLELES[call[i]]
            alleles = [r] + sorted({x, y} - {r})
            idx = sorted(alleles.index(b) for b in (x, y))
            best = int(g[i].max())
            pls = []
            for bi in range(len(alleles)):
                for ai in range(bi + 1):
                    lo, hi = sorted((alleles[ai], alleles[bi]))
                    k = gu.ALLELES.index((lo, hi))
                    pls.append(min((best - int(g[i][k])) * 301 // 25600, 255))
            out.append("%s\t%d\t.\t%s\t%s\t.\t.\t.\tGT:DP:GQ:PL\t%d/%d:%d:%d:%s" % (name, i + 1, "ACGT"[r], ",".join("ACGT"[b] for b in alleles[1:]), idx[0], idx[1], int(depth[t][i]),
                                                                                      int(gq[i]), ",".join(str(p) for p in pls)))
    return out


def test_cli_writes_the_summary_and_the_vcf(tmp_path):
    """The BAM of a run with --genotype_vcf / --genotype_likelihoods holds the same records as one without (all but the XD tag and the header's CL field); the TSV
    equals the binding's summary; every VCF record equals what genotype_calls and the cells of the binding give for the same reads, parameters and seed —
    position, REF from the FASTA (upper-cased; a site whose REF is an IUPAC code is skipped), ALT order, GT, DP, GQ, PL — and there is one record per called site
    whose genotype is not homozygous for the reference base."""
    mapad_amd.lib()
    cli = mbuild.build_cli()
    g = synth.genome(TOTAL, seed=17)
    hap, snps = gu.second_haplotype(g, 50, seed=19)
    batch = pu.concat(synth.reads(g, 500, seed=23, qual_range=(2, 40), damage=DMG, len_range=(25, 110), indel_frac=0.3),
                      synth.reads(hap, 400, 60, seed=24, exo_frac=0.0, qual_range=(20, 40), damage=DMG),
                      pu.hand_made([g[0:40], g[SPLIT - 40:SPLIT], g[TOTAL - 40:TOTAL], with_base(g[5_000:5_060], 30, ord("N"))], qual=31))
    ref = g.copy()
    iupac = [int(x) for x in snps[[3, 30, 60]]]               # IUPAC codes at SNPs of the second haplotype (all on chr1): no record there
    ref[iupac] = ord("R")
    lower = np.arange(300, 900)
    ref[lower] = np.frombuffer(ref[lower].tobytes().lower(), np.uint8)  # lower case in the FASTA: REF is upper-cased
    fa, fq = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fastq")
    with open(fa, "w") as f:
        for name, s in (("chr1", ref[:SPLIT].tobytes().decode()), ("chr2", ref[SPLIT:].tobytes().decode())):
            f.write(f">{name}\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
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
    refs = [ref[:SPLIT], ref[SPLIT:]]
    for name, extra, mode, flt, rule in (("defaults", [], 1, (0, 0, 0), (1, 3.0, 10.0)),
                                         ("unique_filtered", ["--allele_unique", "--allele_min_bq", "20", "--allele_mask5", "2", "--allele_mask3", "1", "--genotype_min_depth", "2",
                                                              "--genotype_min_margin", "1.5", "--genotype_het_penalty", "0.25"], 2, (20, 2, 1), (2, 1.5, 0.25))):
        bam, tsv, vcf = (str(tmp_path / f"{name}.{ext}") for ext in ("bam", "tsv", "vcf"))
        pr = subprocess.run(base + ["-o", bam, "--genotype_vcf", vcf, "--genotype_likelihoods", tsv] + extra, check=True, stderr=subprocess.PIPE, text=True)
        assert "genotype likelihoods (%s)" % ("unique" if mode == 2 else "all") in pr.stderr and "VCF records" in pr.stderr, pr.stderr
        assert _decoded(bam) == plain, name
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            on(ctx, mode, flt)
            ctx.hits_to_records(ctx.map_batch(*batch), *batch, seed=7)
            bound, abound = ctx.genotype_summary(*rule), ctx.allele_summary(rule[0], rule[1])
            cells = [ctx.allele_cells(t, 0, n) for t, n in enumerate(LENGTHS)]
            het = [ctx.genotype_cells(t, 0, n) for t, n in enumerate(LENGTHS)]
            calls = [ctx.genotype_calls(t, 0, n, *rule) for t, n in enumerate(LENGTHS)]
        finally:
            ctx.close()
        head, scalars, rows = _read_tsv(tsv)
        assert head == {"mode": "unique" if mode == 2 else "all", "min_bq": str(flt[0]), "mask5": str(flt[1]), "mask3": str(flt[2]), "min_depth": str(rule[0]),
                        "min_margin_q": str(au.min_margin_q(rule[1])), "het_penalty_q": str(gu.penalty_q(rule[2])), "contigs": "2"}
        assert all(scalars[k] == abound[k] for k in pu.SCALARS) and scalars["reads_seen"] == n_reads and scalars["batches"] == 4 and bound["batches"] == 1 and scalars["reads"] > 0
        assert rows == [{k: c[k] for k in ("name",) + gu.CONTIG_KEYS} for c in bound["contigs"]] and [r["name"] for r in rows] == ["chr1", "chr2"]
        lines = open(vcf).read().splitlines()
        meta, data = [ln for ln in lines if ln.startswith("#")], [ln for ln in lines if not ln.startswith("#")]
        assert meta[0] == "##fileformat=VCFv4.2" and [ln for ln in meta if ln.startswith("##contig")] == [f"##contig=<ID=chr1,length={LENGTHS[0]}>", f"##contig=<ID=chr2,length={LENGTHS[1]}>"]
        assert [re.match(r"##FORMAT=<ID=(\w+),", ln).group(1) for ln in meta if ln.startswith("##FORMAT")] == ["GT", "DP", "GQ", "PL"]
        assert meta[-1].split("\t")[:9] == ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] and len(meta[-1].split("\t")) == 10
        ll, depth = [c[0].astype(np.int64) for c in cells], [c[1].astype(np.int64) for c in cells]
        want = _expected_vcf(["chr1", "chr2"], refs, ll, [h.astype(np.int64) for h in het], depth, rule)
        assert data == want, (name, len(data), len(want), [x for x in zip(data, want) if x[0] != x[1]][:3])
        # the number of records: called sites, not homozygous for the reference base, with an A/C/G/T REF — from the binding's call bytes
        n_records = 0
        for t in range(2):
            code = np.array(["ACGT".find(chr(c).upper()) for c in refs[t]])
            n_records += int(((calls[t][0] != gu.NO_CALL) & (code >= 0) & (calls[t][0] != code)).sum())
        assert len(data) == n_records > 10 and any("," in ln.split("\t")[4] for ln in data) == any(ln.split("\t")[9].startswith("1/2") for ln in data)
        assert any(ln.split("\t")[9].startswith("0/1") for ln in data) and any(ln.split("\t")[9].startswith("1/1") for ln in data)
        assert not any(ln.split("\t")[0] == "chr1" and int(ln.split("\t")[1]) - 1 in iupac for ln in data)
        assert any(calls[0][0][x] != gu.NO_CALL for x in iupac)  # the IUPAC sites: called, skipped
        assert any(300 < int(ln.split("\t")[1]) <= 900 and ln.split("\t")[0] == "chr1" for ln in data) and all(ln.split("\t")[3] in "ACGT" for ln in data)
    # the dependent options need their switch; the VCF needs the FASTA
    for bad in (["--genotype_min_depth", "2"], ["--genotype_min_margin", "2"], ["--genotype_het_penalty", "3"], ["--genotype_vcf", str(tmp_path / "x.vcf"), "--genotype_het_penalty", "-1"],
                ["--genotype_vcf", str(tmp_path / "x.vcf"), "--genotype_min_depth", "0"]):
        assert subprocess.run(base + ["-o", str(tmp_path / "bad.bam")] + bad, stderr=subprocess.PIPE).returncode != 0, bad
