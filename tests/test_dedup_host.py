"""PCR duplicates by alignment coordinates without a GPU: the core's table driven directly (tests/emu/dedup_selftest.cpp, a stand-alone program built with the
address and undefined-behaviour sanitizers), and mapad_dedup_host_* (mapad_amd/csrc/dedup_core.hpp — the source the dedup_* kernels compile too — over the
host's record_coords) against a grouping built independently in numpy from the host records' contig, position, strand and CIGAR (tests/dedup_util.py).  Reads
are mapped by the host build of the kernels' per-read logic (tests/emu)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import synth

import coverage_util as cu
import damage_util as du
import dedup_util as dd
import emu_util
import pileup_util as pu
from kat_util import resolve_params
from parity_util import DAMAGE

_HERE = os.path.dirname(os.path.abspath(__file__))
DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 4242
SPLIT = 250_007
LENGTHS = [SPLIT, 400_000 - SPLIT]
ACGT = np.frombuffer(b"ACGT", np.uint8)
BIG = 300  # members of the large group: more than the histogram's 255


def test_core_selftest_under_sanitizers(tmp_path):
    """insert, find and rehash of dedup_core.hpp in a child process of its own: a table of 8 slots that grows, probing across the table's end, 10 000 random keys
    against a std::map, a rehash that keeps every (key, ordinal, count), the packing's extremes"""
    exe = str(tmp_path / "dedup_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(_HERE, "emu", "dedup_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "dedup selftest ok" in out.stdout, out.stdout + out.stderr


def other(b):
    return ACGT[(int(np.searchsorted(ACGT, b)) + 1) & 3]


def hand_reads(g, rng):
    a, b, c, d, e = 30_000, 40_000, 50_000, 60_000, 70_000
    reads = {
        "fwd": g[a:a + 50], "rev": synth.revcomp(g[a:a + 50]), "fwd_again": g[a:a + 50], "rev_again": synth.revcomp(g[a:a + 50]),
        "len40": g[b:b + 40], "len55": g[b:b + 55],
        "plain60": g[c:c + 60], "ins": np.concatenate([g[c:c + 30], other(g[c + 30])[None], g[c + 30:c + 60]]),
        "plain_d": g[d:d + 60], "del": np.concatenate([g[d:d + 30], g[d + 32:d + 62]]),
        "c1_first": g[0:40], "c1_last": g[SPLIT - 40:SPLIT], "c2_first": g[SPLIT:SPLIT + 40], "c2_last": g[400_000 - 40:400_000],
        "c1_first_again": g[0:40], "c1_last_again": g[SPLIT - 40:SPLIT], "c2_first_again": g[SPLIT:SPLIT + 40], "c2_last_again": g[400_000 - 40:400_000],
    }
    for k in range(BIG):
        reads[f"big{k}"] = g[e:e + 45]
    for k in range(20):
        reads[f"junk{k}"] = ACGT[rng.integers(0, 4, 50)]
    return reads


@pytest.fixture(scope="module")
def world():
    g = synth.genome(400_000, seed=77)
    g[300_000:300_400] = g[100_000:100_400]  # a repeat: reads from it take the coordinate the seeded draw gives them
    idx = mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    rng = np.random.Generator(np.random.PCG64(11))
    hand = hand_reads(g, rng)
    drawn = du.with_duplicates(pu.concat(synth.reads(g, 700, seed=3, qual_range=(20, 40), damage=DMG, len_range=(25, 120), indel_frac=0.2),
                                         synth.reads(g[100_000:100_400], 60, 45, seed=4, exo_frac=0.0)), 500, seed=5)
    full = pu.concat(drawn, pu.hand_made(list(hand.values())))
    n = len(full[2]) - 1
    perm = rng.permutation(n)  # the hand-made reads among the others, so that groups straddle any cut
    batch = du.take(full, perm)
    at = np.empty(n, np.int64)
    at[perm] = np.arange(n)
    where = {name: int(at[n - len(hand) + k]) for k, name in enumerate(hand)}
    return g, idx, params, batch, where


@pytest.fixture(scope="module")
def mapped(world):
    g, idx, params, batch, where = world
    res = emu_util.map_batch(idx, params, *batch)
    recs = mapad_amd.hits_to_records(idx, params, res, *batch, seed=SEED)
    return res, recs


def test_host_flags_equal_the_grouping_of_the_records(world, mapped):
    g, idx, params, batch, where = world
    res, recs = mapped
    acc = mb.DedupHost()
    flags = acc.add(idx, params, res, seed=SEED)
    want, stats = dd.from_records(recs)
    assert np.array_equal(flags, want), np.flatnonzero(flags != want)[:10]
    got = acc.summary()
    dd.assert_stats(got, stats, "host against the grouping")
    n = len(batch[2]) - 1
    assert got["batches"] == 1 and got["reads_seen"] == n and 0 < got["duplicates"] < got["reads_eligible"] < n and got["mark_ms"] == 0.0
    assert got["slots"] >= 2 * got["fragments"] and got["slots"] & (got["slots"] - 1) == 0
    # the batch holds what it is meant to hold
    rec = {name: recs[i] for name, i in where.items()}
    flag = {name: int(flags[i]) for name, i in where.items()}
    later = lambda x, y: (x, y) if where[x] < where[y] else (y, x)  # noqa: E731  (first in the batch, second)
    # the same fragment on both strands: not duplicates of each other, each a duplicate of its own strand's first
    assert rec["fwd"]["mapped"] and rec["rev"]["mapped"] and not rec["fwd"]["reverse"] and rec["rev"]["reverse"]
    assert (rec["fwd"]["tid"], rec["fwd"]["pos"], rec["fwd"]["cigar"]) == (rec["rev"]["tid"], rec["rev"]["pos"], rec["rev"]["cigar"]) == (0, 30_000, "50M")
    for x, y in (("fwd", "fwd_again"), ("rev", "rev_again")):
        first, second = later(x, y)
        assert flag[first] == 0 and flag[second] == 1
    # the same start with different lengths: two molecules
    assert rec["len40"]["pos"] == rec["len55"]["pos"] == 40_000 and (rec["len40"]["cigar"], rec["len55"]["cigar"]) == ("40M", "55M")
    assert flag["len40"] == 0 and flag["len55"] == 0
    # the same span with an insertion: a duplicate
    assert rec["plain60"]["pos"] == rec["ins"]["pos"] == 50_000 and "I" in rec["ins"]["cigar"] and dd.span(rec["ins"]["cigar"]) == dd.span(rec["plain60"]["cigar"]) == 60
    first, second = later("plain60", "ins")
    assert flag[first] == 0 and flag[second] == 1
    # the same start with a deletion: the span differs, no duplicate
    assert rec["plain_d"]["pos"] == rec["del"]["pos"] == 60_000 and "D" in rec["del"]["cigar"] and dd.span(rec["del"]["cigar"]) == 62
    assert flag["plain_d"] == 0 and flag["del"] == 0
    # reads on a contig's first and last base
    for name, tid, pos in (("c1_first", 0, 0), ("c1_last", 0, SPLIT - 40), ("c2_first", 1, 0), ("c2_last", 1, LENGTHS[1] - 40)):
        assert (rec[name]["tid"], rec[name]["pos"]) == (tid, pos) == (rec[name + "_again"]["tid"], rec[name + "_again"]["pos"])
        first, second = later(name, name + "_again")
        assert flag[first] == 0 and flag[second] == 1
    # a group of more than 255 members: the histogram's last bin, exactly one original
    big = sorted(where[f"big{k}"] for k in range(BIG))
    assert all(recs[i]["mapped"] and recs[i]["pos"] == 70_000 for i in big) and flags[big[0]] == 0 and flags[big[1:]].all()
    assert got["histogram"][dd.BINS - 1] == 1 and got["histogram"][0] == 0 and got["histogram"][1] > 0 and got["histogram"][2] > 0
    # unmapped reads are not eligible and never flagged
    junk = [where[f"junk{k}"] for k in range(20)]
    assert not any(recs[i]["mapped"] for i in junk) and not flags[junk].any() and got["reads_eligible"] <= n - 20
    # reads from the repeat (X0 > 1) take part under the coordinate they drew
    assert any(r["mapped"] and r["xt"] == "R" and f for r, f in zip(recs, flags))
    assert [r["duplicate"] for r in recs] == [False] * n  # the host records path does not mark: the flags come from DedupHost


def test_flags_do_not_depend_on_how_the_reads_are_cut_into_batches(world, mapped, monkeypatch):
    g, idx, params, batch, where = world
    res, recs = mapped
    n = len(batch[2]) - 1
    one = mb.DedupHost()
    flags_one = one.add(idx, params, res, seed=SEED)
    monkeypatch.setenv("MAPAD_DEDUP_SLOTS", "64")  # growth between the batches
    three, parts, at = mb.DedupHost(), [], 0
    for end in (n // 3 + 1, 2 * n // 3 + 5, n):
        part = du.take(batch, np.arange(at, end))
        r = emu_util.map_batch(idx, params, *part)
        parts.append(three.add(idx, params, r, seed=int(mapad_amd.lib().mapad_records_seed_at(SEED, at))))
        at = end
    assert np.array_equal(np.concatenate(parts), flags_one)
    s1, s3 = one.summary(), three.summary()
    dd.assert_stats(s3, s1, "three batches against one")
    assert s3["batches"] == 3 and s1["batches"] == 1 and s3["grows"] >= 1 and s1["grows"] == 0
    # groups straddle the cuts: a read of a later batch is flagged for a read of an earlier one
    assert parts[1].sum() > dd.from_records(recs[n // 3 + 1:2 * n // 3 + 5])[0].sum()
    # a batch added twice: the second time every eligible read is a duplicate
    twice = mb.DedupHost()
    first = twice.add(idx, params, res, seed=SEED)
    second = twice.add(idx, params, res, seed=SEED)
    assert np.array_equal(first, flags_one) and not np.array_equal(second, first)
    assert np.array_equal(second, np.array([r["mapped"] for r in recs], np.uint8))
    s = twice.summary()
    assert s["batches"] == 2 and s["reads_seen"] == 2 * n and s["fragments"] == s1["fragments"] and s["duplicates"] == s1["duplicates"] + s1["reads_eligible"]
    # an empty batch counts as a batch and as nothing else
    empty = emu_util.map_batch(idx, params, np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert len(twice.add(idx, params, empty, seed=SEED)) == 0
    s2 = twice.summary()
    assert s2["batches"] == 3 and all(s2[k] == s[k] for k in ("reads_seen", "reads_eligible", "duplicates", "fragments", "slots", "grows"))


@pytest.mark.parametrize("mode", [1, 2])
def test_host_analyses_leave_out_what_skip_names(world, mapped, mode):
    g, idx, params, batch, where = world
    res, recs = mapped
    flags = mb.DedupHost().add(idx, params, res, seed=SEED)
    assert flags.any()
    kept = dd.masked(recs, flags)
    # pileup
    flt = (25, 2, 2)
    acc = mb.PileupHost(idx, mode, *flt).add(params, res, *batch, seed=SEED, skip=flags)
    pu.assert_equal(acc.summary(3, 80), pu.from_records(LENGTHS, kept, batch, mode, *flt), 3, 80, "pileup with skip", counts_of=acc.counts, consensus_of=acc.consensus)
    plain, none = mb.PileupHost(idx, mode, *flt).add(params, res, *batch, seed=SEED), mb.PileupHost(idx, mode, *flt).add(params, res, *batch, seed=SEED, skip=None)
    pu.assert_equal(none.summary(3, 80), plain.summary(3, 80), 3, 80, "pileup, skip=None")
    pu.assert_equal(plain.summary(3, 80), pu.from_records(LENGTHS, recs, batch, mode, *flt), 3, 80, "pileup without skip", counts_of=plain.counts)
    assert acc.summary()["reads"] < plain.summary()["reads"] and acc.summary()["reads_seen"] == plain.summary()["reads_seen"]
    # coverage
    cov = mb.CoverageHost(idx, mode).add(params, res, seed=SEED, skip=flags)
    cu.assert_equal(cov.summary(), cu.from_records(LENGTHS, kept, mode), "coverage with skip", depth_of=cov.depth)
    cov0 = mb.CoverageHost(idx, mode).add(params, res, seed=SEED, skip=None)
    cu.assert_equal(cov0.summary(), cu.from_records(LENGTHS, recs, mode), "coverage, skip=None", depth_of=cov0.depth)
    cu.assert_equal(cov0.summary(), mb.CoverageHost(idx, mode).add(params, res, seed=SEED).summary(), "coverage without skip")
    assert cov.summary()["reads"] < cov0.summary()["reads"] and cov.summary()["reads_seen"] == cov0.summary()["reads_seen"]
    # damage profile
    dmg = mapad_amd.damage_profile_host(idx, params, res, batch[0], batch[2], seed=SEED, mode=mode, skip=flags)
    du.assert_equal(dmg, du.from_records(kept, batch[0], batch[2], mode), "damage with skip")
    dmg0 = mapad_amd.damage_profile_host(idx, params, res, batch[0], batch[2], seed=SEED, mode=mode, skip=None)
    du.assert_equal(dmg0, du.from_records(recs, batch[0], batch[2], mode), "damage, skip=None")
    du.assert_equal(dmg0, mapad_amd.damage_profile_host(idx, params, res, batch[0], batch[2], seed=SEED, mode=mode), "damage without skip")
    assert dmg["reads"] < dmg0["reads"] and dmg["reads_seen"] == dmg0["reads_seen"]


def test_the_boundary(world, mapped):
    g, idx, params, batch, where = world
    res, _ = mapped
    L = mapad_amd.lib()
    names = ("mapad_ctx_set_mark_duplicates", "mapad_ctx_duplicates", "mapad_ctx_duplicates_reset", "mapad_dedup_host_new", "mapad_dedup_host_add",
             "mapad_dedup_host_summary", "mapad_dedup_host_free", "mapad_damage_profile_host_skip", "mapad_coverage_host_add_skip", "mapad_pileup_host_add_skip")
    for name in names:
        assert name in mb.SYMBOLS and hasattr(L, name)
    for name in ("set_mark_duplicates", "duplicates", "duplicates_reset"):
        assert hasattr(mapad_amd.Context, name)
    assert mapad_amd.DedupHost is mb.DedupHost
    out = mb.DuplicatesC()
    assert C.sizeof(out) == 7 * 8 + 256 * 8 + 2 * 8
    assert L.mapad_ctx_set_mark_duplicates(None, 1) == -1 and L.mapad_ctx_duplicates(None, C.byref(out)) == -1 and L.mapad_ctx_duplicates_reset(None) == -1  # MAPAD_ERR_INVALID
    assert L.mapad_dedup_host_new(None) == -1 and L.mapad_dedup_host_summary(None, C.byref(out)) == -1
    assert L.mapad_dedup_host_add(None, None, None, None, 0, None) == -1
    L.mapad_dedup_host_free(None)
    acc = mb.DedupHost()
    assert L.mapad_dedup_host_summary(acc.h, None) == -1
    assert L.mapad_dedup_host_add(acc.h, idx.h, C.byref(params), res._cptr, 0, None) == -1  # reads, and nowhere to write their flags
    assert L.mapad_dedup_host_add(acc.h, None, C.byref(params), res._cptr, 0, None) == -1 and L.mapad_dedup_host_add(acc.h, idx.h, C.byref(params), None, 0, None) == -1
    zero = acc.summary()
    assert zero["reads_seen"] == 0 and zero["batches"] == 0 and zero["fragments"] == 0 and not zero["histogram"].any()
    prof = mb.DamageProfileC()
    assert L.mapad_damage_profile_host_skip(None, None, None, None, None, 0, 1, None, C.byref(prof)) == -1
    assert L.mapad_coverage_host_add_skip(None, None, None, None, 0, None) == -1 and L.mapad_pileup_host_add_skip(None, None, None, None, None, None, None, 0, None) == -1
    for call in (lambda: mb.CoverageHost(idx, 1).add(params, res, seed=SEED, skip=np.zeros(3, np.uint8)),
                 lambda: mb.PileupHost(idx, 1).add(params, res, *batch, seed=SEED, skip=np.zeros(3, np.uint8)),
                 lambda: mapad_amd.damage_profile_host(idx, params, res, batch[0], batch[2], seed=SEED, skip=np.zeros(3, np.uint8))):
        with pytest.raises(ValueError):
            call()  # a skip array that is not one entry per read
