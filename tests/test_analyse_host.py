"""Tracks from alignments without a GPU: mapad_alignment_tracks_host (mapad_amd/csrc/align_core.hpp on the CPU — the source align_count_kernel and
align_build_kernel compile too) against tracks written out by hand and against the rule written once more in Python (tests/analyse_util.py), over the table of
shapes, one read per status class and random consistent alignments; and the core driven directly by tests/emu/align_selftest.cpp, a stand-alone program built
with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import synth

import analyse_util as au
from kat_util import resolve_params
from parity_util import DAMAGE
from test_gpu_panel import TEST_MODEL

_HERE = os.path.dirname(os.path.abspath(__file__))
M, X, I, D = au.OP_MATCH << 24, au.OP_MISMATCH << 24, au.OP_INS << 24, au.OP_DEL << 24


def test_core_selftest_under_sanitizers(tmp_path):
    """the same shapes through align_core.hpp directly, every buffer an exact-size heap copy — in a child process of its own"""
    exe = str(tmp_path / "align_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(_HERE, "emu", "align_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "align selftest ok" in out.stdout, out.stdout + out.stderr


@pytest.fixture(scope="module")
def world():
    g = synth.genome(sum(au.SMALL), seed=5)
    return mapad_amd.Index.build([("c1", g[:au.SMALL[0]]), ("c2", g[au.SMALL[0]:])]), mapad_amd.make_params(resolve_params(DAMAGE))


def _tracks(idx, params, recs, read_lengths, min_mapq=0):
    return mapad_amd.alignment_tracks_host(idx, params, au.offsets_of(read_lengths), *mapad_amd.pack_alignments(recs), min_mapq=min_mapq)


def _one(idx, params, cigar, md, L, reverse=False, **kw):
    t = _tracks(idx, params, [au._rec(cigar, md, reverse=reverse, **kw)], [L])
    assert t["status_class"][0] == 0, au.CLASSES[t["status_class"][0]]
    return [int(w) for w in t["ops"]]


def test_tracks_written_out_by_hand(world):
    idx, params = world
    A, C, G, T, N = (ord(c) << 16 for c in "ACGTN")
    assert _one(idx, params, "4M", "4", 4) == [M | 0, M | 1, M | 2, M | 3]
    assert _one(idx, params, "4M", "4", 4, reverse=True) == [M | 0, M | 1, M | 2, M | 3]
    # a mismatch carries the reference base in read orientation at the position in the read as sequenced: SEQ index 0 of a reverse record is the read's last base
    assert _one(idx, params, "4M", "0A3", 4) == [X | A | 0, M | 1, M | 2, M | 3]
    assert _one(idx, params, "4M", "0A3", 4, reverse=True) == [M | 0, M | 1, M | 2, X | T | 3]
    assert _one(idx, params, "4M", "3c0", 4) == [M | 0, M | 1, M | 2, X | C | 3]
    assert _one(idx, params, "4M", "3c0", 4, reverse=True) == [X | G | 0, M | 1, M | 2, M | 3]
    assert _one(idx, params, "17M", "10A0C5", 17)[9:13] == [M | 9, X | A | 10, X | C | 11, M | 12]
    # 5^AC0T3: the deletion stands behind read position 4 (the model starts at the read's end: found on the way down)
    assert _one(idx, params, "5M2D4M", "5^AC0T3", 9) == [M | 0, M | 1, M | 2, M | 3, M | 4, D | A | 4, D | C | 4, X | T | 5, M | 6, M | 7, M | 8]
    assert _one(idx, params, "5M2D4M", "5^AC0T3", 9, reverse=True) == [M | 0, M | 1, M | 2, X | A | 3, D | G | 3, D | T | 3, M | 4, M | 5, M | 6, M | 7, M | 8]
    # an insertion consumes read positions and carries no base; next to a deletion either way round
    assert _one(idx, params, "2M2I1D2M", "2^G2", 6) == [M | 0, M | 1, I | 2, I | 3, D | G | 3, M | 4, M | 5]
    assert _one(idx, params, "2M1D2I2M", "2^G2", 6) == [M | 0, M | 1, D | G | 1, I | 2, I | 3, M | 4, M | 5]
    # = and X are not trusted over MD
    assert _one(idx, params, "2=1X1=", "4", 4) == [M | 0, M | 1, M | 2, M | 3]
    assert _one(idx, params, "4=", "1N2", 4) == [M | 0, X | N | 1, M | 2, M | 3]
    # a model that starts in the middle of the read: a deletion behind the start carries the position in front of it
    mid = mapad_amd.make_params(resolve_params(TEST_MODEL))
    assert _one(idx, mid, "1M1D5M", "1^A5", 6) == [M | 0, D | A | 0, M | 1, M | 2, M | 3, M | 4, M | 5]
    assert _one(idx, mid, "5M1D1M", "5^A1", 6) == [M | 0, M | 1, M | 2, M | 3, M | 4, D | A | 5, M | 5]


def test_an_ambiguity_code_in_md_becomes_the_reference_base(world):
    """MD carries the original symbol of a reference position that held an ambiguity code; this path takes what MD says"""
    idx, params = world
    N = ord("N") << 16
    assert _one(idx, params, "3M", "1N1", 3) == [M | 0, X | N | 1, M | 2]
    assert _one(idx, params, "3M", "1N1", 3, reverse=True) == [M | 0, X | N | 1, M | 2]
    assert _one(idx, params, "3M", "0R2", 3, reverse=True)[2] == X | ord("Y") << 16 | 2


@pytest.mark.parametrize("model", ["ss", "test_model"])
def test_the_table_of_shapes(world, model):
    idx, _ = world
    params = mapad_amd.make_params(resolve_params(DAMAGE if model == "ss" else TEST_MODEL))
    table = au.shapes(au.SMALL)
    names, recs, lens = [t[0] for t in table], [t[1] for t in table], [t[2] for t in table]
    counts = au.assert_tracks(_tracks(idx, params, recs, lens, min_mapq=10), recs, lens, au.SMALL, min_mapq=10, start_at_end=model == "ss", names=names)
    assert all(counts[k] >= 1 for k in au.CLASSES), counts
    # each read alone gives the same (nothing leaks from one read into the next)
    for name, rec, L in table[::7]:
        au.assert_tracks(_tracks(idx, params, [rec], [L], min_mapq=10), [rec], [L], au.SMALL, min_mapq=10, start_at_end=model == "ss", names=[name])


def test_random_alignments_and_the_mapq_threshold(world):
    idx, params = world
    pairs = au.random_alignments(np.random.default_rng(3), 600, au.SMALL)
    recs, lens = [p[0] for p in pairs], [p[1] for p in pairs]
    assert any("D" in r["cigar"] and r["flags"] & 0x10 for r in recs) and any("I" in r["cigar"] for r in recs) and max(len(r["md"]) for r in recs) > 64
    for min_mapq in (0, 30):
        counts = au.assert_tracks(_tracks(idx, params, recs, lens, min_mapq=min_mapq), recs, lens, au.SMALL, min_mapq=min_mapq)
        assert counts["ok"] + counts["below_min_mapq"] == len(recs) and (counts["below_min_mapq"] > 0) == (min_mapq > 0)


def test_empty_batch_and_bad_arguments(world):
    idx, params = world
    t = mapad_amd.alignment_tracks_host(idx, params, np.zeros(1, np.uint64), *mapad_amd.pack_alignments([]))
    assert len(t["hits"]) == 0 and list(t["hit_begin"]) == [0] and sum(t["class_counts"].values()) == 0
    with pytest.raises(ValueError):
        mapad_amd.alignment_tracks_host(idx, params, au.offsets_of([4, 4]), *mapad_amd.pack_alignments([au._rec("4M", "4")]))
    with pytest.raises(mapad_amd.MapadError):
        _tracks(idx, params, [au._rec("4M", "4")], [4], min_mapq=256)
