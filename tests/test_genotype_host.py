"""The diploid genotype likelihoods without a GPU: the core driven directly (tests/emu/genotype_selftest.cpp, a stand-alone program built with the address
and undefined-behaviour sanitizers), the table of rounded pair values against numpy float64, and the host path (mapad_allele_host_* with genotypes on, over
mapad_amd/csrc/genotype_core.hpp — the source genotype_kernel and genotype_call_kernel compile too) against het cells, genotype calls, GQ and per-contig
statistics built independently in numpy from the host records (tests/genotype_util.py).  Reads are mapped by the host build of the kernels' per-read logic."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import synth

import allele_util as au
import emu_util
import genotype_util as gu
import pileup_util as pu
from kat_util import resolve_params
from parity_util import DAMAGE, IGNORE_BQ

_HERE = os.path.dirname(os.path.abspath(__file__))
DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 717
SPLIT = 6_001
LENGTHS = [SPLIT, 12_000 - SPLIT]
RULES = [(1, 3.0, 0.0), (2, 0.5, 10.0)]  # (min_depth, min_margin in bits, het penalty in bits)
FILTER = (25, 3, 2)
MODELS = {"ss": (DAMAGE, 256), "ignore_bq": (IGNORE_BQ, 1)}


def make(model):
    return mapad_amd.make_params(resolve_params(model))


def test_core_selftest_under_sanitizers(tmp_path):
    """the strand map, the pair value's rounding and identities, the table's layout, the call rule on ties, the penalty, min_depth, GQ / PL clamps and int64
    margins near +-2^31, a backward read, the text's end and a missing table (nothing written) — in a child process of its own"""
    exe = str(tmp_path / "genotype_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(_HERE, "emu", "genotype_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "genotype selftest ok" in out.stdout, out.stdout + out.stderr


def test_table_rows_equal_the_float64_restatement():
    """Every row compared is log2(0.5 * 2^s_x + 0.5 * 2^s_y) in numpy float64 from the f32 model values, rounded as the library rounds: exact, except where the
    float64 value lies within 2^-12 of a rounding tie (there +-1 unit; such rows stay under 1 % of those compared).  A pair's value lies between its two
    alleles' quantised values within 1 unit and never more than 256 units (one bit) below the larger of the two."""
    compared = near_tie_rows = 0
    for name, (model, nq) in MODELS.items():
        p = make(model)
        for L in (50, 21):
            for pos in (0, 1, L // 2, L - 2, L - 1):
                for q in (0, 2, 30, 93):
                    for to in range(4):
                        row = mapad_amd.genotype_quantized_row(p, L, pos, q, to)
                        assert row.dtype == np.int16 and row.shape == (6,)
                        want, near = gu.restated_row(gu.model_values(p, L, pos, q, to, nq))
                        compared += 1
                        near_tie_rows += any(near)
                        for k in range(6):
                            assert abs(int(row[k]) - want[k]) <= (1 if near[k] else 0), (name, L, pos, q, to, k, int(row[k]), want[k])
                        al = mapad_amd.allele_quantized_row(p, L, pos, q, to).astype(int)
                        for k, (x, y) in enumerate(gu.PAIRS):
                            lo, hi = min(al[x], al[y]), max(al[x], al[y])
                            assert lo - 1 <= int(row[k]) <= hi + 1 and int(row[k]) >= hi - 256, (name, L, pos, q, to, k, int(row[k]), lo, hi)
                        other = mapad_amd.genotype_quantized_row(p, L, pos, (q + 17) % 41, to)
                        assert np.array_equal(other, row) == (nq == 1), (name, L, pos, q, to)
    print("rows compared %d, rows with a value within 2^-12 of a rounding tie %d" % (compared, near_tie_rows))
    assert compared == 2 * 2 * 5 * 4 * 4 and near_tie_rows * 100 < compared
    # a deaminated T near the read's 5' end: C/T heterozygote and C homozygote are close; in the interior the het is far better than the hom C
    p = make(DAMAGE)
    for pos, close in ((0, True), (25, False)):
        het_ct = int(mapad_amd.genotype_quantized_row(p, 50, pos, 30, 3)[4])
        hom_c = int(mapad_amd.allele_quantized_row(p, 50, pos, 30, 3)[1])
        assert (het_ct - hom_c < 2 * 256) == close, (pos, het_ct, hom_c)


def test_the_numpy_call_rule_on_hand_set_cells():
    """Pins the test helper only — genotype_util.calls, the numpy restatement the other tests compare the library against — and runs no product code: the
    library's own rule meets the same hand-set cells in tests/emu/genotype_selftest.cpp and the restatement in the parity tests below.  By hand: ties (first in order, margin 0: no call), the penalty flipping a het to a hom,
    min_depth, GQ and PL clamps, int64 margins near +-2^31"""
    i32 = np.iinfo(np.int32)
    ll = np.array([[-10, -800, -900, -1000], [-10, -800, -900, -1000], [-7, -7, -900, -900], [i32.max, i32.min, i32.min, i32.min], [i32.min] * 4, [-10, -800, -900, -1000]], np.int64)
    het = np.array([[-5, -400, -500, -2000, -2000, -2000], [-300, -400, -500, -2000, -2000, -2000], [-300] * 6, [i32.min] * 6, [i32.min] * 5 + [i32.min + 1],
                    [-5, -400, -500, -2000, -2000, -2000]], np.int64)
    depth = np.array([3, 3, 2, 1, 1, 3])
    c, m, gq, pl = gu.calls(ll, het, depth, 1, 1, 0)
    assert list(c) == [4, 0, 255, 0, 9, 4] and list(m) == [5, 290, 0, 2 ** 32 - 1, 1, 5] and list(gq) == [0, 3, 0, 99, 0, 0]
    assert list(pl[0]) == [0, 9, 10, 11, 0, 4, 5, 23, 23, 23] and pl[3].max() == 255 and pl[3][0] == 0
    c, m, gq, _ = gu.calls(ll, het, depth, 1, 1, 5)    # the penalty makes AA and AC equal: the first in order leads with margin 0
    assert c[0] == 255 and m[0] == 0 and gq[0] == 0
    c, m, _, _ = gu.calls(ll, het, depth, 1, 1, 6)     # ... and one unit more flips the het to the hom
    assert c[0] == 0 and m[0] == 1 and c[4] == 255 and m[4] == 0
    c, _, _, _ = gu.calls(ll, het, depth, 3, 1, 0)
    assert list(c) == [4, 0, 255, 255, 255, 4]
    c, m, _, pl = gu.calls(ll, het, depth, 1, 1, i32.max)
    assert c[3] == 0 and m[3] == 2 ** 32 - 1 and pl[3][9] == 255
    assert gu.penalty_q(10.0) == 2560 and gu.penalty_q(0.0) == 0 and gu.penalty_q(0.001) == 1


@pytest.fixture(scope="module")
def world():
    g = synth.genome(12_000, seed=41)
    g[5_000:5_200] = g[2_000:2_200]  # a repeat: mode 2 drops reads that mode 1 counts
    return g, mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])


@pytest.fixture(scope="module")
def batch(world):
    g = world[0]
    hap, _ = gu.second_haplotype(g, 50, seed=5)
    ends = pu.hand_made([g[0:40], g[SPLIT - 40:SPLIT], g[SPLIT:SPLIT + 40], g[12_000 - 40:12_000], synth.revcomp(g[12_000 - 45:12_000]), synth.revcomp(g[SPLIT - 33:SPLIT])], qual=30)
    return pu.concat(synth.reads(g, 300, seed=7, qual_range=(2, 40), damage=DMG, len_range=(55, 75), indel_frac=0.3),
                     synth.reads(hap, 300, 60, seed=9, exo_frac=0.0, qual_range=(20, 40), damage=DMG),
                     synth.reads(g[2_000:2_200], 40, 40, seed=8, exo_frac=0.0, damage=DMG), ends)


@pytest.mark.parametrize("model", list(MODELS))
def test_host_path_equals_the_table_built_from_the_records(world, batch, model):
    g, idx = world
    p = make(MODELS[model][0])
    res = emu_util.map_batch(idx, p, *batch)
    recs = mapad_amd.hits_to_records(idx, p, res, *batch, seed=SEED)
    rows, arows = gu.Rows(p), au.Rows(p)
    n = len(batch[2]) - 1
    skip = (np.arange(n) % 3 == 0).astype(np.uint8)
    for mode, flt, sk in ((1, (0, 0, 0), None), (2, FILTER, None), (1, (0, 0, 0), skip)):
        acc = mb.AlleleHost(idx, mode, *flt, genotypes=True).add(p, res, *batch, seed=SEED, skip=sk)
        want = gu.from_records(p, LENGTHS, recs, batch, mode, *flt, rows=rows, allele_rows=arows, skip=sk)
        for rule in RULES:
            gu.assert_equal(acc, want, rule, f"{model}, mode {mode}, filters {flt}, skip {sk is not None}, rule {rule}")
        if mode == 2:  # what it rides on is unchanged by it
            plain = mb.AlleleHost(idx, mode, *flt).add(p, res, *batch, seed=SEED, skip=sk)
            au.assert_same_accumulators(acc, plain, LENGTHS, [(1, 3.0)], "allele read-outs with and without genotypes")
            assert plain.genotype_summary()["on"] == 0 and not plain.genotype_cells(0, 0, 50).any() and (plain.genotype_calls(0, 0, 50)[0] == 255).all()
    s = acc.genotype_summary(1, 3.0, 0.0)  # (the last setting: mode 1, no filters, every third read skipped)
    assert s["batches"] == 1 and s["accumulate_ms"] == 0.0
    assert sum(sum(c["called"][4:]) for c in s["contigs"]) > 0 and sum(sum(c["called"][:4]) for c in s["contigs"]) > 0  # het and hom calls both lead somewhere
    with pytest.raises(mapad_amd.MapadError):  # only before the first add
        mapad_amd.binding._check(mapad_amd.lib().mapad_allele_host_set_genotypes(acc.h, 0), "mapad_allele_host_set_genotypes")
    nan = float("nan")
    for call in (lambda: acc.genotype_summary(0, 3.0, 0.0), lambda: acc.genotype_summary(1, nan, 0.0), lambda: acc.genotype_summary(1, 3.0, nan), lambda: acc.genotype_summary(1, 3.0, -0.5),
                 lambda: acc.genotype_calls(0, 0, 4, 1, 3.0, -1.0), lambda: acc.genotype_calls(0, LENGTHS[0] - 3, 4), lambda: acc.genotype_cells(2, 0, 1), lambda: acc.genotype_cells(0, LENGTHS[0] - 3, 4)):
        with pytest.raises(mapad_amd.MapadError):
            call()


@pytest.mark.parametrize("model", ["ignore_bq", "ss"])
def test_a_fragment_and_its_reverse_complement_add_mirrored_cells(model):
    """One fragment given forward and reverse-complemented (qualities reversed), on a text and on the text's reverse complement: a read that lies forward on
    one lies backward on the other, and the cells of the two texts mirror each other — position x against n - 1 - x, pair k against the pair of the
    complemented alleles (AC <-> GT, AG <-> CT, AT and CG stay), allele a against 3 - a."""
    g = synth.genome(2_000, seed=77)
    n = len(g)
    p = make(MODELS[model][0])
    frag, q = g[700:760].copy(), (np.arange(60) % 30 + 10).astype(np.uint8)
    frag[0], frag[59] = ord("T"), ord("A")  # mismatches at the ends, where the damage model is steep, on both strands
    tables = []
    for text in (g, synth.revcomp(g)):
        idx = mapad_amd.Index.build([("c", text)])
        per_read = []
        for seq, qual in ((frag, q), (synth.revcomp(frag), q[::-1].copy())):
            b = (seq.copy(), qual, np.array([0, 60], np.uint64))
            res = emu_util.map_batch(idx, p, *b)
            recs = mapad_amd.hits_to_records(idx, p, res, *b, seed=SEED)
            acc = mb.AlleleHost(idx, 1, genotypes=True).add(p, res, *b, seed=SEED)
            per_read.append((bool(recs[0]["reverse"]), acc.genotype_cells(0, 0, n), acc.cells(0, 0, n)[0]))
            assert recs[0]["mapped"] and acc.cells(0, 0, n)[1].sum() == 60
        tables.append(per_read)
    for r in range(2):
        (rev_a, het_a, ll_a), (rev_b, het_b, ll_b) = tables[0][r], tables[1][r]
        assert rev_a != rev_b and het_a.any()
        assert np.array_equal(het_a, het_b[::-1][:, gu.STRAND]) and np.array_equal(ll_a, ll_b[::-1, ::-1]), (model, r)
        assert not np.array_equal(het_a, het_b[::-1][:, ::-1])  # (AT and CG do not swap)
    # the two reads of one text: forward and backward over the same columns, different cells (the damage model knows the read's ends)
    assert tables[0][0][0] != tables[0][1][0] and not np.array_equal(tables[0][0][1], tables[0][1][1])


def test_the_boundary(world):
    L = mapad_amd.lib()
    names = ("mapad_ctx_set_genotype_likelihoods", "mapad_ctx_genotype_summary", "mapad_ctx_genotype_cells", "mapad_ctx_genotype_calls", "mapad_ctx_genotype_merge",
             "mapad_genotype_quantized_row", "mapad_allele_host_set_genotypes", "mapad_allele_host_genotype_summary", "mapad_allele_host_genotype_cells",
             "mapad_allele_host_genotype_calls")
    for name in names:
        assert name in mb.SYMBOLS and hasattr(L, name)
    for name in ("set_genotype_likelihoods", "genotype_summary", "genotype_cells", "genotype_calls", "genotype_merge"):
        assert hasattr(mapad_amd.Context, name)
    assert mapad_amd.genotype_quantized_row is mb.genotype_quantized_row and mapad_amd.GENOTYPES == gu.GENOTYPES
    out = mb.GenotypeC()
    assert C.sizeof(mb.GenotypeContigC) == 16 * 8 and C.sizeof(out) == 8 + 8 + 4 * 4 + 8 + 2 * 8
    buf = (C.c_uint32 * 32)()
    f3, f0 = C.c_float(3.0), C.c_float(0.0)
    assert L.mapad_ctx_set_genotype_likelihoods(None, 1) == -1 and L.mapad_ctx_genotype_summary(None, 1, f3, f0, C.byref(out)) == -1
    assert L.mapad_ctx_genotype_cells(None, 0, 0, 4, buf) == -1 and L.mapad_ctx_genotype_calls(None, 0, 0, 4, 1, f3, f0, buf, buf) == -1 and L.mapad_ctx_genotype_merge(None, None) == -1
    assert L.mapad_allele_host_set_genotypes(None, 1) == -1 and L.mapad_allele_host_genotype_summary(None, 1, f3, f0, C.byref(out)) == -1
    assert L.mapad_allele_host_genotype_cells(None, 0, 0, 4, buf) == -1 and L.mapad_allele_host_genotype_calls(None, 0, 0, 4, 1, f3, f0, buf, buf) == -1
    p = make(DAMAGE)
    row = (C.c_int16 * 6)()
    for bad in ((0, 0, 30, 0), (32768, 0, 30, 0), (50, 50, 30, 0), (50, 0, 256, 0), (50, 0, 30, 4)):
        assert L.mapad_genotype_quantized_row(C.byref(p), *bad, row) == -1, bad
    assert L.mapad_genotype_quantized_row(None, 50, 0, 30, 0, row) == -1 and L.mapad_genotype_quantized_row(C.byref(p), 50, 0, 30, 0, None) == -1
    _, idx = world
    acc = mb.AlleleHost(idx, 1, genotypes=True)
    zero = acc.genotype_summary(1, -4.0, 0.0)  # a margin below one unit is one unit: nothing is called where nothing was counted
    assert zero["on"] == 1 and zero["min_margin_q"] == 1 and zero["batches"] == 0
    assert all(c["sites_covered"] == 0 and c["sites_called"] == 0 and c["max_depth"] == 0 and c["margin_sum_q"] == 0 and c["length"] == LENGTHS[t] for t, c in enumerate(zero["contigs"]))
    gt, gq = acc.genotype_calls(1, 0, 5)
    assert (gt == 255).all() and not gq.any() and len(acc.genotype_cells(0, LENGTHS[0], 0)) == 0


def test_the_damage_aware_table_calls_fewer_false_heterozygotes_than_a_zero_damage_table():
    """Meaning, and nothing else.  A 40 kb reference; a second haplotype with a SNP about every 200 bases; reads drawn half from each with the single-stranded
    damage of the preset (f = t = 0.5, d = 0.02, s = 1.0), mean depth about 12; mapped under the damage parameters.  Genotype calls under the library's
    defaults (min_depth 1, margin 3 bits, no het penalty: a prior would push both tables' heterozygotes down alike) at the reference's C and G sites, once under the mapping parameters and once with the cells rebuilt over the same alignments
    from the same parameters with both deamination rates zero.  The damage-aware table calls strictly fewer false heterozygotes, and at least half as many true
    ones — so it does not get there by calling nothing.  Printed beside them, not asserted: the calls from zero-damage het cells beside the damage-aware
    homozygous cells — about the damage-aware table's, because what keeps a deaminated T over a C from being read as C/T is the homozygous C cell, which knows
    that the T is cheap near a read's end; the C/T cell itself rightly gains from the damage model there."""
    g = synth.genome(40_000, seed=53)
    hap, snps = gu.second_haplotype(g, 200, seed=59)
    idx = mapad_amd.Index.build([("chr", g)])
    p = make(DAMAGE)
    p0 = make(dict(DAMAGE, ds_deamination_rate=0.0, ss_deamination_rate=0.0))
    a, b = (synth.reads(h, 4800, 50, seed=s, subst_rate=0.001, exo_frac=0.0, qual_range=(20, 40), damage=DMG) for h, s in ((g, 61), (hap, 62)))
    batch = pu.concat(a, b)
    res = emu_util.map_batch(idx, p, *batch)
    aware = mb.AlleleHost(idx, 1, genotypes=True).add(p, res, *batch, seed=SEED)
    blind = mb.AlleleHost(idx, 1, genotypes=True).add(p0, res, *batch, seed=SEED)  # an accumulator holds the sums of one model: all ten values at zero damage
    n = len(g)
    ll, depth = aware.cells(0, 0, n)
    assert np.array_equal(depth, blind.cells(0, 0, n)[1])  # the same alignments, the same columns
    cg = (g == ord("C")) | (g == ord("G"))
    is_snp = np.zeros(n, bool)
    is_snp[snps] = True
    code = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), np.stack([g, hap]))
    lo, hi = code.min(axis=0), code.max(axis=0)
    pair = np.array([[0, 4, 5, 6], [4, 1, 7, 8], [5, 7, 2, 9], [6, 8, 9, 3]])
    truth = pair[lo, hi]
    rule = (1, 3.0, 0.0)

    def count(call):
        het_call = (call >= 4) & (call != gu.NO_CALL) & cg
        return int((het_call & ~is_snp).sum()), int((het_call & is_snp & (call == truth)).sum())

    call_aware = aware.genotype_calls(0, 0, n, *rule)[0]
    call_mix = gu.calls(ll, blind.genotype_cells(0, 0, n), depth, 1, au.min_margin_q(3.0), 0)[0]  # zero-damage het cells beside the damage-aware homozygous cells (no accumulator holds this; the rule in numpy)
    counts = {"damage-aware": count(call_aware), "zero-damage": count(blind.genotype_calls(0, 0, n, *rule)[0]), "zero-damage het cells only": count(call_mix)}  # (the last: recorded, not asserted)
    for name, (false_het, true_het) in counts.items():
        print("%s table, reference C/G sites: %d false heterozygotes, %d true heterozygotes of %d; mean depth %.2f" % (name, false_het, true_het, int((is_snp & cg).sum()), depth.sum() / n))
    (false_aware, true_aware), (false_blind, true_blind) = counts["damage-aware"], counts["zero-damage"]
    assert false_aware < false_blind
    assert 2 * true_aware >= true_blind and true_blind > 0
    # what the het table itself decides, the homozygous cells being the same on both sides: the two tables' rows differ exactly where the model knows damage,
    # and at some C/G site that changes the call; wherever the call changes between two heterozygotes or between a heterozygote and none, only het cells differ
    het_aware, het_blind = aware.genotype_cells(0, 0, n), blind.genotype_cells(0, 0, n)
    moved = np.flatnonzero((call_aware != call_mix) & cg)
    print("sites whose call the het table alone changes: %d of %d C/G sites with different het cells" % (len(moved), int(((het_aware != het_blind).any(axis=1) & cg).sum())))
    assert len(moved) >= 1 and all((het_aware[x] != het_blind[x]).any() for x in moved)
    ct = mapad_amd.genotype_quantized_row(p, 50, 0, 30, 3).astype(int) - mapad_amd.genotype_quantized_row(p0, 50, 0, 30, 3).astype(int)
    assert ct[4] > 0 and ct[1] == 0 and ct[2] == 0 and ct[5] == 0  # a 5' T: the C/T pair gains from the damage model (P(T | C) is no longer an error's); pairs without C are the same
