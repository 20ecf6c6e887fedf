"""The damage profile without a GPU: mapad_damage_profile_host (mapad_amd/csrc/damage_core.hpp — the source damage_kernel compiles too — over the host's
record_coords) against a table computed independently in numpy from the host records' CIGAR / MD / strand / XT and the input reads (tests/damage_util.py).
Reads are mapped by the host build of the kernels' per-read logic (tests/emu)."""
import ctypes as C

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import synth

import damage_util as du
import emu_util
from kat_util import resolve_params
from parity_util import DAMAGE

DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 4242


def concat(*batches):
    seqs = np.concatenate([b[0] for b in batches])
    quals = np.concatenate([b[1] for b in batches])
    offs, base = [np.zeros(1, np.uint64)], 0
    for b in batches:
        offs.append(b[2][1:] + np.uint64(base))
        base += int(b[2][-1])
    return seqs, quals, np.concatenate(offs)


@pytest.fixture(scope="module")
def world():
    g = synth.genome(150_000, seed=31)
    g[60_000:60_300] = g[20_000:20_300]  # a repeat: reads from it have X0 > 1, so mode 2 drops reads that mode 1 counts
    idx = mapad_amd.Index.build([("c1", g[:70_000]), ("c2", g[70_000:])])
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    return g, idx, params


def mapped(world, batch):
    _, idx, params = world
    return emu_util.map_batch(idx, params, *batch)


def both(world, batch, res, seed, mode):
    """(the library's host path, the numpy table from the host records)"""
    _, idx, params = world
    recs = mapad_amd.hits_to_records(idx, params, res, *batch, seed=seed)
    return mb.damage_profile_host(idx, params, res, batch[0], batch[2], seed=seed, mode=mode), du.from_records(recs, batch[0], batch[2], mode)


@pytest.fixture(scope="module")
def damaged(world):
    g = world[0]
    batch = concat(synth.reads(g, 2400, seed=7, qual_range=(20, 40), damage=DMG, len_range=(20, 70), indel_frac=0.3),
                   synth.reads(g[20_000:20_300], 200, 40, seed=8, exo_frac=0.0, damage=DMG))
    return batch, mapped(world, batch)


@pytest.mark.parametrize("mode", [1, 2])
def test_host_profile_equals_the_table_decoded_from_the_records(world, damaged, mode):
    batch, res = damaged
    got, want = both(world, batch, res, SEED, mode)
    du.assert_equal(got, want)
    n = len(batch[2]) - 1
    assert got["reads_seen"] == n and 0 < got["reads"] < n and got["batches"] == 1
    assert got["insertions"] > 0 and got["deletions"] > 0          # gapped alignments are in it
    assert int(got["counts"][0].sum()) <= got["aligned_bases"] and int(got["counts"][1].sum()) <= got["aligned_bases"]
    lens = np.diff(batch[2].astype(np.int64))
    assert (lens < 64).any() and int(got["counts"].sum()) > got["aligned_bases"]  # bases of short reads are in both tables
    assert got["skipped_bases"] == 0


def test_unique_mode_counts_fewer_reads(world, damaged):
    batch, res = damaged
    all_reads, _ = both(world, batch, res, SEED, 1)
    unique, _ = both(world, batch, res, SEED, 2)
    assert unique["reads"] < all_reads["reads"] and unique["reads_seen"] == all_reads["reads_seen"]
    assert (unique["counts"] <= all_reads["counts"]).all()


def test_reads_with_n_are_skipped_not_counted(world):
    g = world[0]
    seqs, quals, offsets = synth.reads(g, 600, 50, seed=9, qual_range=(20, 40), damage=DMG, exo_frac=0.0)
    seqs = seqs.copy()
    rng = np.random.Generator(np.random.PCG64(3))
    at = offsets[:-1].astype(np.int64)[::2] + rng.integers(8, 42, len(offsets[:-1][::2]))
    seqs[at] = ord("N")  # one N in every second read
    batch = (seqs, quals, offsets)
    res = mapped(world, batch)
    for mode in (1, 2):
        got, want = both(world, batch, res, SEED, mode)
        du.assert_equal(got, want)
        assert got["skipped_bases"] > 0


def test_two_batches_add_up_to_their_concatenation(world, damaged):
    g, idx, params = world
    a, res_a = damaged
    b = synth.reads(g, 700, seed=10, qual_range=(20, 40), damage=DMG, len_range=(25, 60), indel_frac=0.2)
    res_b = mapped(world, b)
    ab = concat(a, b)
    res_ab = mapped(world, ab)
    n_a = len(a[2]) - 1
    seed_b = int(mapad_amd.lib().mapad_records_seed_at(SEED, n_a))
    for mode in (1, 2):
        one = mb.damage_profile_host(idx, params, res_ab, ab[0], ab[2], seed=SEED, mode=mode)
        two = mb.damage_profile_host(idx, params, res_a, a[0], a[2], seed=SEED, mode=mode)
        two = mb.damage_profile_host(idx, params, res_b, b[0], b[2], seed=seed_b, mode=mode, into=two)
        du.assert_equal(two, one)
        assert two["batches"] == 2 and one["batches"] == 1


def test_damage_shows_at_the_five_prime_end_and_only_with_damage(world, damaged):
    """No tolerance invented: with damage the C>T frequency at 5' position 1 exceeds the one at position 20; without, the two differ by no more than the A>G
    frequencies of the same two positions do (a substitution the damage model knows nothing of)."""
    g = world[0]
    batch, res = damaged
    c = both(world, batch, res, SEED, 1)[0]["counts"]
    assert du.freq(c, 0, 0, "C", "T") > du.freq(c, 0, 19, "C", "T")
    assert du.freq(c, 1, 0, "C", "T") > du.freq(c, 1, 19, "C", "T")  # single-stranded library: C>T at the 3' end as well
    # (both differences are sampling noise of ~500 C / A per position, so which is larger depends on the seed: this one was checked through this host path)
    plain = synth.reads(g, 2400, 50, seed=16, qual_range=(20, 40), damage=None)
    c = both(world, plain, mapped(world, plain), SEED, 1)[0]["counts"]
    assert abs(du.freq(c, 0, 0, "C", "T") - du.freq(c, 0, 19, "C", "T")) <= abs(du.freq(c, 0, 0, "A", "G") - du.freq(c, 0, 19, "A", "G"))


def test_the_boundary():
    L = mapad_amd.lib()
    for name in ("mapad_ctx_set_damage_profile", "mapad_ctx_damage_profile", "mapad_ctx_damage_profile_reset", "mapad_damage_profile_host"):
        assert name in mb.SYMBOLS and hasattr(L, name)
    for name in ("set_damage_profile", "damage_profile", "reset_damage_profile"):
        assert hasattr(mapad_amd.Context, name)
    out = mb.DamageProfileC()
    assert C.sizeof(out) == 2 * 32 * 16 * 8 + 7 * 8 + 8
    assert L.mapad_ctx_set_damage_profile(None, 1) == -1 and L.mapad_ctx_damage_profile(None, C.byref(out)) == -1 and L.mapad_ctx_damage_profile_reset(None) == -1
    assert L.mapad_damage_profile_host(None, None, None, None, None, 0, 1, C.byref(out)) == -1  # MAPAD_ERR_INVALID


def test_mode_zero_is_not_a_host_mode(world, damaged):
    _, idx, params = world
    batch, res = damaged
    with pytest.raises(mapad_amd.MapadError):
        mb.damage_profile_host(idx, params, res, batch[0], batch[2], seed=SEED, mode=0)
