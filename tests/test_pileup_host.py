"""The pileup without a GPU: mapad_pileup_host_* (mapad_amd/csrc/pileup_core.hpp — the source pileup_kernel and pileup_call_kernel compile too — over the host's
record_coords) against counts, skip counters, calls and per-contig statistics built independently in numpy from the host records' contig, position, CIGAR,
strand and XT and the reads (tests/pileup_util.py).  Reads are mapped by the host build of the kernels' per-read logic (tests/emu)."""
import ctypes as C

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import synth

import emu_util
import pileup_util as pu
from kat_util import resolve_params
from parity_util import DAMAGE

DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 909
SPLIT = 70_001
LENGTHS = [SPLIT, 150_000 - SPLIT]
FILTERS = [(0, 0, 0), (30, 3, 2)]  # (min_bq, mask5, mask3)
RULES = [(1, 0), (3, 80)]          # (min_depth, min_percent)
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def world():
    g = synth.genome(150_000, seed=31)
    g[60_000:60_300] = g[20_000:20_300]  # a repeat: reads from it have X0 > 1, so mode 2 drops reads that mode 1 counts
    idx = mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    return g, idx, params


def code(b):
    return int(np.searchsorted(ACGT, b))


def other(b):
    """another base: A -> C -> G -> T -> A"""
    return ACGT[(code(b) + 1) & 3]


def with_base(read, at, b):
    read = read.copy()
    read[at] = b
    return read


# The hand-made reads, by name -> (read, qualities or None for 30 everywhere).  TIE / THREE: the positions of c1 where two of four / one of four reads carry another base.
TIE, THREE, QUAL_AT, SHORT_AT, EMPTY_AT = 8_000, 9_000, 5_000, 6_000, 50_000


def hand_reads(g):
    q = np.full(40, 30, np.uint8)
    q[10] = 29  # one below the threshold of 30; position 11 is exactly at it
    reads = {
        "c1_first": (g[0:40], None), "c1_last": (g[SPLIT - 40:SPLIT], None), "c2_first": (g[SPLIT:SPLIT + 40], None), "c2_last": (g[150_000 - 40:150_000], None),
        "c1_last_rev": (synth.revcomp(g[SPLIT - 45:SPLIT]), None),
        "fwd_del": (np.concatenate([g[1_000:1_030], g[1_032:1_060]]), None), "fwd_ins": (np.concatenate([g[1_500:1_530], other(g[1_530])[None], g[1_530:1_560]]), None),
        "rev_del": (synth.revcomp(np.concatenate([g[3_000:3_030], g[3_032:3_060]])), None),
        "rev_ins": (synth.revcomp(np.concatenate([g[3_500:3_530], other(g[3_530])[None], g[3_530:3_560]])), None),
        "with_n": (with_base(g[4_000:4_050], 20, ord("N")), None), "with_n_rev": (with_base(synth.revcomp(g[4_500:4_550]), 20, ord("N")), None),
        "short": (g[SHORT_AT:SHORT_AT + 22], None), "quals": (g[QUAL_AT:QUAL_AT + 40], q),
    }
    for k in range(2):
        reads[f"tie_ref{k}"] = (g[TIE - 20:TIE + 20], None)
        reads[f"tie_alt{k}"] = (with_base(g[TIE - 20:TIE + 20], 20, other(g[TIE])), None)
    for k in range(3):
        reads[f"three_ref{k}"] = (g[THREE - 20:THREE + 20], None)
    reads["three_alt"] = (synth.revcomp(with_base(g[THREE - 20:THREE + 20], 20, other(g[THREE]))), None)  # (on the reverse strand: its base is complemented back)
    return reads


def hand_batch(g):
    reads = hand_reads(g)
    seqs, quals, offs = pu.hand_made([r for r, _ in reads.values()], qual=30)
    quals = quals.copy()
    for k, (_, q) in enumerate(reads.values()):
        if q is not None:
            quals[int(offs[k]):int(offs[k + 1])] = q
    return list(reads), (seqs, quals, offs)


@pytest.fixture(scope="module")
def hand(world):
    g, idx, params = world
    names, batch = hand_batch(g)
    res = emu_util.map_batch(idx, params, *batch)
    recs = mapad_amd.hits_to_records(idx, params, res, *batch, seed=SEED)
    return names, batch, res, recs


@pytest.fixture(scope="module")
def mapped(world, hand):
    g, idx, params = world
    batch = pu.concat(synth.reads(g, 1300, seed=7, qual_range=(20, 40), damage=DMG, len_range=(20, 150), indel_frac=0.3),
                      synth.reads(g[20_000:20_300], 150, 40, seed=8, exo_frac=0.0, damage=DMG), hand[1])
    res = emu_util.map_batch(idx, params, *batch)
    recs = mapad_amd.hits_to_records(idx, params, res, *batch, seed=SEED)
    return batch, res, recs


def host(world, res, batch, mode, flt=(0, 0, 0), seed=SEED, into=None):
    _, idx, params = world
    acc = into if into is not None else mb.PileupHost(idx, mode, *flt)
    return acc.add(params, res, *batch, seed=seed)


def check_against_numpy(acc, want, what):
    for rule in RULES:
        pu.assert_equal(acc.summary(*rule), want, *rule, what=f"{what}, rule {rule}", counts_of=acc.counts, consensus_of=acc.consensus)
    for t, c in enumerate(want["counts"]):  # windows that start in the middle of a contig, on covered ground
        d = c.sum(axis=1)
        for start in (int(np.argmax(d)), LENGTHS[t] - 17):
            n = min(700, LENGTHS[t] - start)
            assert d[start] > 0 and np.array_equal(acc.counts(t, start, n).astype(np.int64), c[start:start + n]), (what, t, start)
            assert np.array_equal(acc.consensus(t, start, n, 2, 60), pu.consensus(c[start:start + n], 2, 60)), (what, t, start)
    assert len(acc.counts(0, LENGTHS[0], 0)) == 0 and len(acc.consensus(0, LENGTHS[0], 0)) == 0


@pytest.mark.parametrize("flt", FILTERS + [(0, 15, 10)])
def test_hand_made_reads(world, hand, flt):
    g = world[0]
    names, batch, res, recs = hand
    rec = dict(zip(names, recs))
    assert all(r["mapped"] and r["xt"] == "U" for r in recs), [n for n, r in rec.items() if not r["mapped"] or r["xt"] != "U"]
    # the reads are where and how they were meant to be
    assert (rec["c1_first"]["tid"], rec["c1_first"]["pos"]) == (0, 0) and (rec["c2_first"]["tid"], rec["c2_first"]["pos"]) == (1, 0)
    assert (rec["c1_last"]["tid"], rec["c1_last"]["pos"]) == (0, SPLIT - 40) and (rec["c2_last"]["tid"], rec["c2_last"]["pos"]) == (1, LENGTHS[1] - 40)
    for name, op, reverse in (("fwd_del", "D", False), ("fwd_ins", "I", False), ("rev_del", "D", True), ("rev_ins", "I", True), ("with_n", "M", False), ("with_n_rev", "M", True),
                              ("three_alt", "M", True), ("c1_last_rev", "M", True)):
        assert op in rec[name]["cigar"] and rec[name]["reverse"] == reverse, (name, rec[name])
    for mode in (1, 2):
        acc = host(world, res, batch, mode, flt)
        want = pu.from_records(LENGTHS, recs, batch, mode, *flt)
        check_against_numpy(acc, want, f"hand-made, mode {mode}, filters {flt}")
        s = acc.summary()
        assert s["reads"] == s["reads_seen"] == len(names) and s["batches"] == 1 and (s["mode"], s["min_base_quality"], s["mask5"], s["mask3"]) == (mode,) + flt
        assert s["columns_not_acgt"] == 2 and s["deleted_columns"] == 4 and s["insertions"] == 2
        col = lambda at: acc.counts(0, at, 1)[0]  # noqa: E731
        if flt == (0, 0, 0):
            assert s["columns_masked"] == 0 and s["columns_low_quality"] == 0
            assert col(0)[code(g[0])] == 1 and col(SPLIT - 1)[code(g[SPLIT - 1])] == 2 and acc.counts(1, 0, 1)[0].sum() == 1 and acc.counts(1, LENGTHS[1] - 1, 1)[0].sum() == 1
            assert col(4_020).sum() == 0 and col(4_500 + 29).sum() == 0 and col(4_019).sum() == 1  # the N of either strand is in no cell
            assert col(QUAL_AT + 10).sum() == 1 and col(QUAL_AT + 11).sum() == 1
            # the call rule on these cells: two of four, three of four, none
            tie, three = col(TIE), col(THREE)
            assert sorted(tie) == [0, 0, 2, 2] and tie[code(g[TIE])] == 2 and tie[code(other(g[TIE]))] == 2
            assert sorted(three) == [0, 0, 1, 3] and three[code(g[THREE])] == 3 and three[code(other(g[THREE]))] == 1
            call = lambda at, d, p: chr(acc.consensus(0, at, 1, d, p)[0])  # noqa: E731
            ref = chr(g[THREE])
            assert call(TIE, 1, 0) == "N" and call(TIE, 4, 50) == "N"                      # a tie is no call, whatever the thresholds
            assert call(THREE, 4, 0) == ref and call(THREE, 5, 0) == "N"                   # depth exactly min_depth, and one below it
            assert call(THREE, 1, 75) == ref and call(THREE, 1, 76) == "N"                 # 3 of 4 is 75 percent
            assert call(THREE, 1, 0) == ref and call(THREE, 1, 100) == "N"                 # min_percent 0 with a unique maximum
            assert col(EMPTY_AT).sum() == 0 and call(EMPTY_AT, 1, 0) == "N"                # nothing there
            assert call(TIE - 1, 4, 100) == chr(g[TIE - 1]) and call(TIE - 1, 5, 100) == "N"
        elif flt == (30, 3, 2):
            assert s["columns_low_quality"] == 1 and col(QUAL_AT + 10).sum() == 0 and col(QUAL_AT + 11).sum() == 1  # 29 is below the threshold, 30 is at it
            assert s["columns_masked"] > 0 and col(0).sum() == 0 and col(2).sum() == 0 and col(3).sum() == 1 and col(37).sum() == 1 and col(38).sum() == 0
            assert col(SPLIT - 1).sum() == 0 and col(SPLIT - 3).sum() == 1  # c1_last masks the 2 bases of its 3' end there, c1_last_rev the 3 of its 5' end
        else:
            assert not acc.counts(0, SHORT_AT, 22).any()  # 22 bases under masks of 15 + 10: masked entirely, and still a read
            assert col(15).sum() == 1 and col(14).sum() == 0 and col(29).sum() == 1 and col(30).sum() == 0


@pytest.mark.parametrize("flt", FILTERS)
@pytest.mark.parametrize("mode", [1, 2])
def test_host_pileup_equals_the_table_built_from_the_records(world, mapped, mode, flt):
    batch, res, recs = mapped
    acc = host(world, res, batch, mode, flt)
    want = pu.from_records(LENGTHS, recs, batch, mode, *flt)
    check_against_numpy(acc, want, f"mode {mode}, filters {flt}")
    got = acc.summary(3, 80)
    n = len(batch[2]) - 1
    assert got["reads_seen"] == n and 0 < got["reads"] < n and got["batches"] == 1 and got["accumulate_ms"] == 0.0
    assert got["deleted_columns"] > 0 and got["insertions"] > 0 and got["columns_not_acgt"] == 2
    assert [c["name"] for c in got["contigs"]] == ["c1", "c2"] and [c["length"] for c in got["contigs"]] == LENGTHS
    assert all(0 < c["sites_called"] <= c["sites_deep"] <= c["sites_covered"] < c["length"] and sum(c["called"]) == c["sites_called"] for c in got["contigs"])
    if flt != (0, 0, 0):
        assert got["columns_masked"] > 0 and got["columns_low_quality"] > 0
    # the world is what it is meant to be: tracks longer than one pass of a wavefront, deletions on both strands
    counted = [r for r in recs if r["mapped"] and (mode == 1 or r["xt"] == "U")]
    assert any(sum(int(k) for k, _ in pu._CIGAR.findall(r["cigar"])) > 64 for r in counted)
    assert {r["reverse"] for r in counted if "D" in r["cigar"]} == {False, True}
    if mode == 2:
        assert got["reads"] < sum(1 for r in recs if r["mapped"])


def test_two_batches_add_up_to_their_concatenation(world):
    g, idx, params = world
    a = synth.reads(g, 400, seed=10, qual_range=(20, 40), damage=DMG, len_range=(25, 90), indel_frac=0.3)
    b = pu.concat(synth.reads(g, 250, seed=11, qual_range=(20, 40), damage=DMG, len_range=(25, 60), indel_frac=0.2), synth.reads(g[20_000:20_300], 60, 40, seed=12, exo_frac=0.0))
    ab = pu.concat(a, b)
    res_a, res_b, res_ab = (emu_util.map_batch(idx, params, *x) for x in (a, b, ab))
    seed_b = int(mapad_amd.lib().mapad_records_seed_at(SEED, len(a[2]) - 1))
    for mode in (1, 2):
        one = host(world, res_ab, ab, mode, (25, 2, 2))
        two = host(world, res_b, b, mode, (25, 2, 2), seed=seed_b, into=host(world, res_a, a, mode, (25, 2, 2)))
        s1, s2 = one.summary(2, 70), two.summary(2, 70)
        pu.assert_equal(s2, s1, 2, 70, f"mode {mode}")
        assert s2["batches"] == 2 and s1["batches"] == 1
        for t, n in enumerate(LENGTHS):
            assert np.array_equal(one.counts(t, 0, n), two.counts(t, 0, n)) and np.array_equal(one.consensus(t, 0, n, 2, 70), two.consensus(t, 0, n, 2, 70))


def test_the_boundary(world):
    L = mapad_amd.lib()
    names = ("mapad_ctx_set_pileup", "mapad_ctx_pileup", "mapad_ctx_pileup_counts", "mapad_ctx_pileup_consensus", "mapad_ctx_pileup_reset", "mapad_ctx_pileup_merge",
             "mapad_pileup_host_new", "mapad_pileup_host_add", "mapad_pileup_host_summary", "mapad_pileup_host_counts", "mapad_pileup_host_consensus", "mapad_pileup_host_free")
    for name in names:
        assert name in mb.SYMBOLS and hasattr(L, name)
    for name in ("set_pileup", "pileup", "pileup_counts", "pileup_consensus", "pileup_reset", "pileup_merge"):
        assert hasattr(mapad_amd.Context, name)
    assert mapad_amd.PileupHost is mb.PileupHost
    out = mb.PileupC()
    assert C.sizeof(mb.PileupContigC) == 13 * 8 and C.sizeof(out) == 8 + 8 + 6 * 4 + 9 * 8 + 2 * 8
    buf = (C.c_uint32 * 16)()
    assert L.mapad_ctx_set_pileup(None, 1, 0, 0, 0) == -1 and L.mapad_ctx_pileup(None, 1, 0, C.byref(out)) == -1 and L.mapad_ctx_pileup_reset(None) == -1  # MAPAD_ERR_INVALID
    assert L.mapad_ctx_pileup_counts(None, 0, 0, 4, buf) == -1 and L.mapad_ctx_pileup_consensus(None, 0, 0, 4, 1, 0, buf) == -1 and L.mapad_ctx_pileup_merge(None, None) == -1
    h = C.c_void_p()
    assert L.mapad_pileup_host_new(None, 1, 0, 0, 0, C.byref(h)) == -1 and L.mapad_pileup_host_add(None, None, None, None, None, None, None, 0) == -1
    assert L.mapad_pileup_host_summary(None, 1, 0, C.byref(out)) == -1 and L.mapad_pileup_host_counts(None, 0, 0, 4, buf) == -1
    assert L.mapad_pileup_host_consensus(None, 0, 0, 4, 1, 0, buf) == -1
    L.mapad_pileup_host_free(None)
    _, idx, _ = world
    for bad in ((0, 0, 0, 0), (3, 0, 0, 0), (1, 256, 0, 0), (1, 0, 65536, 0), (1, 0, 0, 65536)):  # mode 0 is not a host mode; filters beyond a quality / a read position
        with pytest.raises(mapad_amd.MapadError):
            mb.PileupHost(idx, *bad)
    acc = mb.PileupHost(idx, 1)
    for call in (lambda: acc.counts(0, LENGTHS[0] - 3, 4), lambda: acc.counts(2, 0, 1), lambda: acc.consensus(0, LENGTHS[0] - 3, 4), lambda: acc.consensus(0, 0, 4, 0, 50),
                 lambda: acc.consensus(0, 0, 4, 1, 101), lambda: acc.summary(0, 0), lambda: acc.summary(1, 101)):  # windows that leave their contig; min_depth 0; min_percent 101
        with pytest.raises(mapad_amd.MapadError):
            call()
    zero = acc.summary(1, 0)
    assert zero["reads_seen"] == 0 and zero["batches"] == 0 and all(c["sites_covered"] == 0 and c["max_depth"] == 0 and c["base_sum"] == [0] * 4 for c in zero["contigs"])
    assert bytes(acc.consensus(1, 0, 5)) == b"NNNNN"


def test_planted_variants_show_in_the_consensus():
    """The condition of tests/test_gpu_pileup.py's planted-variant test, met without a GPU, on the same genome, reads and seed: reads drawn from a copy of 20 kbp
    that differs from the genome in one base of 997, mapped to the original, give a consensus (min_depth 3, min_percent 80) equal to the copy wherever there is a
    call, and there is one at 90 % of the stretch at least — by the numpy table and by the host path alike."""
    g = synth.genome(400_000, seed=77)
    g[300_000:300_400] = g[100_000:100_400]
    split = 250_007
    idx = mapad_amd.Index.build([("c1", g[:split]), ("c2", g[split:])])
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    copy, at, batch = pu.planted(g)
    res = emu_util.map_batch(idx, params, *batch)
    recs = mapad_amd.hits_to_records(idx, params, res, *batch, seed=99)
    want = pu.from_records([split, 400_000 - split], recs, batch, 1)
    cons = pu.consensus(want["counts"][0][pu.PLANT_START:pu.PLANT_START + pu.PLANT_LEN], 3, 80)
    pu.assert_planted(copy, at, cons, g[pu.PLANT_START:pu.PLANT_START + pu.PLANT_LEN])
    acc = mb.PileupHost(idx, 1).add(params, res, *batch, seed=99)
    assert np.array_equal(acc.consensus(0, pu.PLANT_START, pu.PLANT_LEN, 3, 80), cons)
