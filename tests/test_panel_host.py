"""The SNP panel without a GPU: the core driven directly (tests/emu/panel_selftest.cpp, a stand-alone program built with the address and undefined-behaviour
sanitizers), and mapad_snp_panel_host_* (mapad_amd/csrc/panel_core.hpp — the source panel_kernel and panel_call_kernel compile too — over the host's
record_coords) against strand-split counts, counters, calls and row statistics built independently in numpy from the host records' contig, position, CIGAR,
strand and XT and the reads (tests/panel_util.py).  Reads are mapped by the host build of the kernels' per-read logic (tests/emu).  The command line maps on a
GPU only, so what it writes is compared in tests/test_gpu_panel.py; how it reads a .snp file and names contigs is checked here through `mapad-amd panel`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import build as mbuild
from mapad_amd import synth

import emu_util
import panel_util as pn
import pileup_util as pu
from kat_util import resolve_params
from parity_util import DAMAGE

_HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 99
FILTERS = [(0, 0, 0), (30, 3, 2)]  # (min_bq, mask5, mask3)


def test_core_selftest_under_sanitizers(tmp_path):
    """the 64-probe search at 0, 1, 63, 64, 65, 4097 and more slots with targets before, on and behind them; 130 slots inside one read on either strand;
    insertions, deletions on slots, filters; the text's end; the call rule at n = 0, at min_depth exactly, on ties and on either kind of transition — in a child
    process of its own"""
    exe = str(tmp_path / "panel_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(_HERE, "emu", "panel_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "panel selftest ok" in out.stdout, out.stdout + out.stderr


@pytest.fixture(scope="module")
def world():
    g = pn.world_genome()
    idx = mapad_amd.Index.build([("c1", g[:pn.SPLIT]), ("c2", g[pn.SPLIT:])])
    return g, idx, mapad_amd.make_params(resolve_params(DAMAGE)), pn.panel(g)


@pytest.fixture(scope="module")
def mapped(world):
    g, idx, params, _ = world
    batch = pn.mixed_batch(g, 1500, seed=5)
    res = emu_util.map_batch(idx, params, *batch)
    return batch, res, mapad_amd.hits_to_records(idx, params, res, *batch, seed=SEED)


def host(world, res, batch, mode, flt=(0, 0, 0), seed=SEED, into=None, p=None, skip=None):
    _, idx, params, panel = world
    acc = into if into is not None else mb.SnpPanelHost(idx, mode, *pn.args(panel if p is None else p), *flt)
    return acc.add(params, res, *batch, seed=seed, skip=skip)


@pytest.mark.parametrize("flt", FILTERS)
@pytest.mark.parametrize("mode", [1, 2])
def test_host_panel_equals_the_table_built_from_the_records(world, mapped, mode, flt):
    g, idx, params, p = world
    batch, res, recs = mapped
    acc = host(world, res, batch, mode, flt)
    want = pn.from_records(pn.LENGTHS, recs, batch, p, mode, *flt)
    pn.assert_equal(acc.summary, acc.counts, acc.calls, want, pn.LENGTHS, p, f"mode {mode}, filters {flt}")
    got = acc.summary()
    n = len(batch[2]) - 1
    assert got["reads_seen"] == n and 0 < got["reads_on_panel"] < got["reads"] < n and got["batches"] == 1 and got["accumulate_ms"] == 0.0
    assert (got["mode"], got["min_base_quality"], got["mask5"], got["mask3"]) == (mode,) + flt and got["n_slots"] < got["n_rows"] == len(p["tid"])
    assert got["rows_unplaced"] == 5 and got["rows_bad_alleles"] == 4 and got["columns_deleted"] >= 2 and got["columns_not_acgt"] >= 1
    if flt == (0, 0, 0):
        assert got["columns_masked"] == 0 and got["columns_low_quality"] == 0
    else:
        assert got["columns_masked"] > 0 and got["columns_low_quality"] > 0
    # the world is what it is meant to be: a counted read over more than 64 slots, deletions over a slot on both strands, reads on the contigs' ends
    counted = [r for r in recs if r["mapped"] and (mode == 1 or r["xt"] == "U")]
    dense = [r for r in counted if r["tid"] == 0 and pn.DENSE_START <= r["pos"] and r["pos"] + 100 <= pn.DENSE_START + pn.DENSE_LEN and "150M" in r["cigar"]]
    assert {r["reverse"] for r in dense} == {False, True}
    assert {r["reverse"] for r in counted if "D" in r["cigar"] and r["tid"] == 0 and pn.DENSE_START <= r["pos"] < pn.DENSE_START + pn.DENSE_LEN} == {False, True}
    if flt == (0, 0, 0):
        ends = {(int(t), int(x)): i for i, (t, x) in enumerate(zip(p["tid"], p["pos0"])) if (int(t), int(x)) in ((0, 0), (0, pn.SPLIT - 1), (1, 0), (1, pn.LENGTHS[1] - 1))}
        assert len(ends) == 4 and all(acc.counts(i, 1).sum() >= 1 for i in ends.values())
    # rows at one position share their counts and keep their alleles
    for x in pn.PAIRS_AT:
        a, b = np.flatnonzero((p["tid"] == 0) & (p["pos0"] == x))[:2]
        assert np.array_equal(acc.counts(a, 1), acc.counts(b, 1)) and p["alt"][a] != p["alt"][b]


@pytest.mark.parametrize("flt", FILTERS)
def test_strands_add_up_to_the_pileup_and_single_strand_uses_the_documented_one(world, mapped, flt):
    g, idx, params, p = world
    batch, res, _ = mapped
    ok = pn.placed(pn.LENGTHS, p)
    for mode in (1, 2):
        acc = host(world, res, batch, mode, flt)
        pile = mb.PileupHost(idx, mode, *flt).add(params, res, *batch, seed=SEED)
        per_contig = [pile.counts(t, 0, n) for t, n in enumerate(pn.LENGTHS)]
        counts = acc.counts(0, len(ok))
        for i in np.flatnonzero(ok):
            assert np.array_equal(counts[i].sum(axis=0), per_contig[int(p["tid"][i])][int(p["pos0"][i])]), (mode, i)
        assert not counts[~ok].any()
        # majority calls under single_strand, from the one strand's counts alone
        rule = dict(call=1, min_depth=1, transitions=2, seed=3)
        calls = acc.calls(0, len(ok), rule)
        checked = {"CT": 0, "GA": 0}
        for i in np.flatnonzero(ok):
            r, a = int(pu._CODE[p["ref"][i]]), int(pu._CODE[p["alt"][i]])
            if max(r, a) > 3 or r == a or {r, a} not in ({1, 3}, {0, 2}):
                continue
            c = counts[i][1] if {r, a} == {1, 3} else counts[i][0]  # C/T: the reverse strand; G/A: the forward strand
            if c[r] == c[a]:
                assert (calls[i] == ord("9")) == (c[r] == 0)
                continue
            assert calls[i] == (ord("2") if c[r] > c[a] else ord("0")), (mode, i, counts[i])
            checked["CT" if {r, a} == {1, 3} else "GA"] += 1
        assert min(checked.values()) > 100, checked


def test_calls_are_tied_to_rows_seeds_and_nothing_else(world):
    g, idx, params, p = world
    a = synth.reads(g[:60_000], 350, seed=10, qual_range=(20, 40), damage=pn.DMG, len_range=(25, 90), indel_frac=0.3)
    b = pu.concat(synth.reads(g[:60_000], 250, seed=11, qual_range=(20, 40), damage=pn.DMG, len_range=(25, 60), indel_frac=0.2), synth.reads(g[100_000:100_400], 40, 40, seed=12, exo_frac=0.0))
    ab = pu.concat(a, b)
    res_a, res_b, res_ab = (emu_util.map_batch(idx, params, *x) for x in (a, b, ab))
    seed_b = int(mapad_amd.lib().mapad_records_seed_at(SEED, len(a[2]) - 1))
    n_rows = len(p["tid"])
    rule = dict(call=0, min_depth=1, transitions=0, seed=77)
    for mode in (1, 2):
        one = host(world, res_ab, ab, mode, (25, 2, 2))
        two = host(world, res_b, b, mode, (25, 2, 2), seed=seed_b, into=host(world, res_a, a, mode, (25, 2, 2)))
        s1, s2 = one.summary(rule), two.summary(rule)
        assert {k: v for k, v in s1.items() if k != "batches"} == {k: v for k, v in s2.items() if k != "batches"} and (s1["batches"], s2["batches"]) == (1, 2)
        assert np.array_equal(one.counts(0, n_rows), two.counts(0, n_rows)) and np.array_equal(one.calls(0, n_rows, rule), two.calls(0, n_rows, rule))
        assert np.array_equal(one.calls(0, n_rows, rule), one.calls(0, n_rows, dict(rule)))  # the same seed: the same calls
        other = one.calls(0, n_rows, dict(rule, seed=78))
        assert (other != one.calls(0, n_rows, rule)).any() and np.array_equal(other == ord("9"), one.calls(0, n_rows, rule) == ord("9"))  # another seed: other draws, the same rows
    # the reads in reverse order (mode 2: a uniquely mapped read's reported hit does not depend on its place in the batch)
    reads = [ab[0][int(ab[2][i]):int(ab[2][i + 1])] for i in range(len(ab[2]) - 1)][::-1]
    quals = np.concatenate([ab[1][int(ab[2][i]):int(ab[2][i + 1])] for i in range(len(ab[2]) - 1)][::-1])
    seqs, _, offs = pu.hand_made(reads)
    rev = (seqs, quals, offs)
    back = host(world, emu_util.map_batch(idx, params, *rev), rev, 2, (25, 2, 2))
    fwd = host(world, res_ab, ab, 2, (25, 2, 2))
    assert np.array_equal(back.counts(0, n_rows), fwd.counts(0, n_rows)) and np.array_equal(back.calls(0, n_rows, rule), fwd.calls(0, n_rows, rule))
    assert fwd.summary(rule)["rows_called"] > 100


def test_the_draw_follows_the_allele_fractions(world):
    """Over the rows with 0 < n_ref < n the number of ref calls is a sum of independent Bernoulli(n_ref / n) draws: within 5 standard deviations of its mean
    sum(n_ref / n), the variance being sum((n_ref / n)(1 - n_ref / n)).  A panel of its own — every position of 20 kbp with the transition partner as alt — under
    damaged reads drawn from those 20 kbp gives well over the 300 such rows asked for (deaminated C and G beside intact ones)."""
    g, idx, params, _ = world
    lo, n = pu.PLANT_START, 20_000
    p = {"tid": np.zeros(n, np.int32), "pos0": np.arange(lo, lo + n, dtype=np.uint64), "ref": g[lo:lo + n].copy(), "alt": pn._next(g[lo:lo + n], 2)}
    batch = synth.reads(g[lo:lo + n], 1500, seed=21, qual_range=(20, 40), damage=pn.DMG, len_range=(20, 150), indel_frac=0.1)
    acc = host(world, emu_util.map_batch(idx, params, *batch), batch, 1, p=p)
    counts = acc.counts(0, n).astype(np.int64)
    for seed in (0, 1, 2**63 + 5):
        rule = dict(call=0, min_depth=1, transitions=0, seed=seed)
        calls, _, seen = pn.calls(pn.LENGTHS, p, counts, **rule)
        assert np.array_equal(acc.calls(0, n, rule), calls)
        mixed = [i for i, s in enumerate(seen) if s is not None and 0 < s[0] < s[1]]
        frac = np.array([seen[i][0] / seen[i][1] for i in mixed])
        assert len(mixed) >= 300, len(mixed)
        refs = int((calls[mixed] == ord("2")).sum())
        assert abs(refs - frac.sum()) <= 5 * np.sqrt((frac * (1 - frac)).sum()), (seed, len(mixed), refs, frac.sum())


def test_planted_variants_are_called_alt(world):
    """Reads drawn from a copy of 20 kbp that differs from the genome in one base of 997, mapped to the original: at the planted sites — rows whose alt is the
    planted base — majority calls at min_depth 3 say alt wherever there is a call, and there is one at 90 % of them at least."""
    g, idx, params, p = world
    _, at, batch = pu.planted(g)
    acc = host(world, emu_util.map_batch(idx, params, *batch), batch, 1)
    calls = acc.calls(0, len(p["tid"]), dict(call=1, min_depth=3))[p["planted"]]
    assert len(calls) == len(at) and (calls != ord("2")).all()
    assert int((calls == ord("0")).sum()) * 10 >= 9 * len(at), calls


def test_the_boundary(world):
    L = mapad_amd.lib()
    names = ("mapad_ctx_set_snp_panel", "mapad_ctx_snp_panel", "mapad_ctx_snp_panel_counts", "mapad_ctx_snp_panel_calls", "mapad_ctx_snp_panel_reset", "mapad_ctx_snp_panel_merge",
             "mapad_snp_panel_host_new", "mapad_snp_panel_host_add", "mapad_snp_panel_host_add_skip", "mapad_snp_panel_host_summary", "mapad_snp_panel_host_counts",
             "mapad_snp_panel_host_calls", "mapad_snp_panel_host_free")
    for name in names:
        assert name in mb.SYMBOLS and hasattr(L, name)
    for name in ("set_snp_panel", "snp_panel", "snp_panel_counts", "snp_panel_calls", "snp_panel_reset", "snp_panel_merge"):
        assert hasattr(mapad_amd.Context, name)
    assert mapad_amd.SnpPanelHost is mb.SnpPanelHost
    assert C.sizeof(mb.SnpPanelRuleC) == 24 and C.sizeof(mb.SnpPanelC) == 16 + 24 + 24 * 8 + 16
    out, rule, buf = mb.SnpPanelC(), mb.snp_panel_rule(), (C.c_uint32 * 64)()
    assert L.mapad_ctx_set_snp_panel(None, 1, 0, None, None, None, None, 0, 0, 0) == -1 and L.mapad_ctx_snp_panel(None, C.byref(rule), C.byref(out)) == -1  # MAPAD_ERR_INVALID
    assert L.mapad_ctx_snp_panel_counts(None, 0, 1, buf) == -1 and L.mapad_ctx_snp_panel_calls(None, 0, 1, C.byref(rule), buf) == -1
    assert L.mapad_ctx_snp_panel_reset(None) == -1 and L.mapad_ctx_snp_panel_merge(None, None) == -1
    assert L.mapad_snp_panel_host_summary(None, C.byref(rule), C.byref(out)) == -1 and L.mapad_snp_panel_host_counts(None, 0, 1, buf) == -1
    L.mapad_snp_panel_host_free(None)
    g, idx, params, p = world
    one = (np.array([0], np.int32), np.array([5], np.uint64), b"A", b"C")
    for bad in ((0,) + one, (3,) + one, (1,) + one + (256,), (1,) + one + (0, 65536), (1,) + one + (0, 0, 65536), (1, np.zeros(0, np.int32), np.zeros(0, np.uint64), b"", b"")):
        with pytest.raises(mapad_amd.MapadError):  # mode 0 is not a host mode; filters beyond a quality / a read position; a panel of no rows
            mb.SnpPanelHost(idx, *bad)
    with pytest.raises(ValueError):
        mb.SnpPanelHost(idx, 1, [0, 0], [5], b"A", b"C")
    acc = mb.SnpPanelHost(idx, 1, *pn.args(p))
    n = len(p["tid"])
    for call in (lambda: acc.counts(n - 3, 4), lambda: acc.calls(n, 1), lambda: acc.calls(0, 4, dict(min_depth=0)), lambda: acc.calls(0, 4, dict(call=2)),
                 lambda: acc.summary(dict(transitions=3))):  # windows that leave the panel; min_depth 0; an unknown call or transitions setting
        with pytest.raises(mapad_amd.MapadError):
            call()
    zero = acc.summary()
    assert zero["reads_seen"] == 0 and zero["batches"] == 0 and zero["rows_called"] == 0 and zero["rows"] == n and zero["max_depth"] == 0
    assert bytes(acc.calls(0, 5)) == b"99999" and len(acc.counts(n, 0)) == 0 and len(acc.calls(n, 0)) == 0


def test_cli_reads_a_snp_file_and_names_contigs(tmp_path):
    """`mapad-amd panel` places the rows as `map --snp_panel` does: the exact name, "chr" + name, 23 / 24 / 90 as X / Y / MT (also with chr, and chrM); a
    chromosome that names no contig is unplaced, not an error; a malformed line is refused with its number"""
    mapad_amd.lib()
    cli = mbuild.build_cli()
    g = synth.genome(3_000, seed=3)

    def index_of(names):
        d = tmp_path / ("ref_" + "_".join(names))
        d.mkdir()
        fa = str(d / "ref.fa")
        with open(fa, "w") as f:
            for k, name in enumerate(names):
                f.write(f">{name}\n{g[500 * k:500 * (k + 1)].tobytes().decode()}\n")
        subprocess.check_call([cli, "index", "-g", fa])
        return fa

    def placed(fa, lines):
        snp = str(tmp_path / "panel.snp")
        open(snp, "w").write("".join(ln + "\n" for ln in lines))
        pr = subprocess.run([cli, "panel", "-g", fa, "--snp_panel", snp], capture_output=True, text=True)
        return pr, [tuple(ln.split("\t")) for ln in pr.stdout.splitlines()]

    lines = ["rs1 1 0.0 10 A C", "rs2\t2\t0.01\t500\tG\tT", "  rs3   23  0.5  1  C  T  ", "rs4 24 0 7 a g", "rs5 90 0 3 T C", "rs6 X 0 2 A G", "rs7 chr2 0 9 A G", "rs8 7 0 9 A G",
             "rs9 1 0 501 A C", "rs10 1 0 0 A C", ""]
    pr, rows = placed(index_of(["chr1", "2", "chrX", "Y", "chrM", "chr2"]), lines)
    assert pr.returncode == 0, pr.stderr
    assert rows == [("rs1", "0", "9"), ("rs2", "1", "499"), ("rs3", "2", "0"), ("rs4", "3", "6"), ("rs5", "4", "2"), ("rs6", "2", "1"), ("rs7", "5", "8"), ("rs8", "-1", "8"),
                    ("rs9", "0", "500"), ("rs10", "-1", "0")]  # (rs9: past its contig's end — the library leaves it unplaced; rs10: position 0 is no position)
    pr, rows = placed(index_of(["1", "chr1", "X", "MT"]), ["a 1 0 1 A C", "b chr1 0 1 A C", "c 23 0 1 A C", "d 90 0 1 A C", "e chrX 0 1 A C"])
    assert rows == [("a", "0", "0"), ("b", "1", "0"), ("c", "2", "0"), ("d", "3", "0"), ("e", "-1", "0")]  # the exact name first
    fa = index_of(["c1"])
    for bad, number in ((["rs1 c1 0 10 A C", "rs2 c1 0 10 A"], 2), (["rs1 c1 0 x A C"], 1), (["rs1 c1 0 10 A C", "", "rs3 c1 0 10 AC G"], 3), (["rs1 c1 zero 10 A C"], 1),
                        (["rs1 c1 0 10 A C extra"], 1), (["rs1 c1 0 -5 A C"], 1)):
        pr, _ = placed(fa, bad)
        assert pr.returncode != 0 and f"line {number}:" in pr.stderr, (bad, pr.stderr)
    pr, _ = placed(fa, [""])
    assert pr.returncode != 0 and "no panel rows" in pr.stderr
