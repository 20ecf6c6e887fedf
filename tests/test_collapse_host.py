"""Duplicate collapsing without a GPU: the host build of mapad_amd/csrc/collapse_core.hpp (tests/emu/collapse_selftest.cpp — the very functions the two grouping
kernels call) against an independent numpy grouping of (length, bases, qualities) tuples, and the argument checks of the two C entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emu", "collapse_selftest.cpp")
_lib = None


def selftest_lib():
    """tests/emu/collapse_selftest.cpp, built on demand with g++ (like emu_util.heap_selftest_lib)"""
    global _lib
    if _lib is None:
        out = os.path.join(_HERE, "emu", "_build", "libcollapse_selftest.so")
        csrc = os.path.join(_HERE, "..", "mapad_amd", "csrc")
        deps = [_SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", out + f".tmp{os.getpid()}", _SRC])
            os.replace(out + f".tmp{os.getpid()}", out)
        L = C.CDLL(out)
        L.collapse_group_host.restype = C.c_int
        L.collapse_group_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def pack(reads):
    """[(bases bytes, qualities list / bytes)] -> seqs, quals, offsets"""
    seqs = np.frombuffer(b"".join(bytes(r[0]) for r in reads), np.uint8).copy() if reads else np.zeros(0, np.uint8)
    quals = np.frombuffer(b"".join(bytes(r[1]) for r in reads), np.uint8).copy() if reads else np.zeros(0, np.uint8)
    offsets = np.zeros(len(reads) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(r[0]) for r in reads])
    return seqs, quals, offsets


def numpy_grouping(seqs, quals, offsets, ignore_qual=False):
    """dup_of by a dictionary of (length, bases, qualities) tuples: the lowest index represents"""
    n = len(offsets) - 1
    first, dup_of = {}, np.zeros(n, np.uint32)
    for i in range(n):
        a, b = int(offsets[i]), int(offsets[i + 1])
        key = (b - a, seqs[a:b].tobytes(), b"" if ignore_qual else quals[a:b].tobytes())
        dup_of[i] = first.setdefault(key, i)
    return dup_of


def core_grouping(seqs, quals, offsets, ignore_qual=False, key_bits=64):
    n = len(offsets) - 1
    dup_of, stats = np.zeros(max(n, 1), np.uint32), np.zeros(3, np.uint64)
    s = np.ascontiguousarray(np.concatenate([seqs, np.zeros(8, np.uint8)]))  # (never read: the core stops at a read's last byte)
    q = np.ascontiguousarray(np.concatenate([quals, np.zeros(8, np.uint8)]))
    rc = selftest_lib().collapse_group_host(s.ctypes.data, q.ctypes.data, offsets.ctypes.data, n, int(ignore_qual), key_bits, dup_of.ctypes.data, stats.ctypes.data)
    assert rc == 0
    return dup_of[:n], [int(x) for x in stats]


def _random_reads(rng, n, lens=(30, 60), alphabet=b"ACGT", quals=(2, 12, 23, 37)):
    out = []
    for _ in range(n):
        L = int(rng.integers(lens[0], lens[1] + 1))
        out.append((bytes(rng.choice(np.frombuffer(alphabet, np.uint8), L)), bytes(rng.choice(np.array(quals, np.uint8), L))))
    return out


def _batches():
    rng = np.random.Generator(np.random.PCG64(17))
    base = _random_reads(rng, 400)
    mixed = base + [base[int(k)] for k in rng.integers(0, len(base), 700)]
    mixed = [mixed[int(k)] for k in rng.permutation(len(mixed))]
    a = (b"ACGTACGTACGTACGTACGTACGTACGTACGTAC", bytes([30] * 34))
    return {
        "empty": [],
        "one": [a],
        "same_bases_other_qualities": [a, (a[0], bytes([30] * 33 + [31])), a, (a[0], bytes([12] * 34)), (a[0], bytes([30] * 33 + [31]))],
        "proper_prefix": [a, (a[0][:33], a[1][:33]), (a[0][:32], a[1][:32]), a, (a[0][:33], a[1][:33]), (a[0] + b"A", a[1] + bytes([30]))],
        "mixed_lengths_with_duplicates": mixed,
        "one_read_10000_times": [a] * 10000,
        "no_duplicate": _random_reads(rng, 3000),
        "short_reads_and_tails": [(b"A", b"\x05"), (b"AC", b"\x05\x05"), (b"A", b"\x05"), (b"ACG", b"\x05\x05\x05"), (b"ACGTA", b"\x05" * 5), (b"ACGTA", b"\x05" * 5), (b"ACGTC", b"\x05" * 5)],
    }


BATCHES = _batches()


@pytest.mark.parametrize("name", list(BATCHES))
def test_core_groups_like_numpy(name):
    seqs, quals, offsets = pack(BATCHES[name])
    want = numpy_grouping(seqs, quals, offsets)
    got, stats = core_grouping(seqs, quals, offsets)
    assert np.array_equal(got, want)
    n = len(want)
    sizes = np.bincount(want, minlength=max(n, 1))
    assert stats[0] == int((want == np.arange(n)).sum())
    assert stats[1] == int(sizes[sizes >= 2].sum())
    assert stats[2] == 0  # no 64-bit collision in a test
    if name == "one_read_10000_times":
        assert stats[0] == 1 and stats[1] == 10000
    if name == "no_duplicate":
        assert stats[0] == n and stats[1] == 0


@pytest.mark.parametrize("key_bits", [1, 3, 6])
@pytest.mark.parametrize("name", list(BATCHES))
def test_colliding_keys_never_merge_different_reads(name, key_bits):
    """The key cut down to a few bits: most candidates collide.  The grouping is numpy's or finer, and no group holds two different reads."""
    seqs, quals, offsets = pack(BATCHES[name])
    want = numpy_grouping(seqs, quals, offsets)
    got, stats = core_grouping(seqs, quals, offsets, key_bits=key_bits)
    n = len(want)
    assert np.array_equal(want[got], want), "a read was merged with a different read"  # the representative is a read of the same numpy group ...
    assert (got <= np.arange(n)).all() and np.array_equal(got[got], got)                 # ... with a lower index, and is itself searched
    if n:
        assert stats[0] == int((got == np.arange(n)).sum()) >= int((want == np.arange(n)).sum())
    if name in ("mixed_lengths_with_duplicates", "no_duplicate"):
        assert stats[2] > 0, "the collision path was not taken"
    if name == "one_read_10000_times":
        assert np.array_equal(got, want)  # one key: nothing to collide with


@pytest.mark.parametrize("key_bits", [64, 2])
def test_ignored_qualities_do_not_separate_reads(key_bits):
    for name in ("same_bases_other_qualities", "mixed_lengths_with_duplicates", "proper_prefix"):
        seqs, quals, offsets = pack(BATCHES[name])
        rng = np.random.Generator(np.random.PCG64(5))
        quals = np.where(rng.random(quals.size) < 0.3, quals + 1, quals).astype(np.uint8)
        with_q = numpy_grouping(seqs, quals, offsets)
        want = numpy_grouping(seqs, quals, offsets, ignore_qual=True)
        assert not np.array_equal(with_q, want)
        got, _ = core_grouping(seqs, quals, offsets, ignore_qual=True, key_bits=key_bits)
        if key_bits == 64:
            assert np.array_equal(got, want)
        else:
            assert np.array_equal(want[got], want) and np.array_equal(got[got], got)
    seqs, quals, offsets = pack(BATCHES["same_bases_other_qualities"])
    got, stats = core_grouping(seqs, quals, offsets, ignore_qual=True)
    assert np.array_equal(got, np.zeros(5, np.uint32)) and stats[:2] == [1, 5]


def test_entry_points_refuse_a_null_context():
    L = mapad_amd.lib()
    out = np.zeros(8, np.uint64)
    assert L.mapad_ctx_set_collapse_duplicates(None, 1) == -1  # MAPAD_ERR_INVALID
    assert L.mapad_last_collapse_info(None, out.ctypes.data_as(C.c_void_p)) == -1
    assert "mapad_ctx_set_collapse_duplicates" in mb.SYMBOLS and "mapad_last_collapse_info" in mb.SYMBOLS
    assert hasattr(mapad_amd.Context, "set_collapse_duplicates") and hasattr(mapad_amd.Context, "collapse_info")
