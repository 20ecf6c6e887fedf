"""The backward-only search step (mapad_amd/csrc/search_core.hpp: search_step<.., BWD = true>) against the general step, without a GPU.

tests/emu/bwd_step.cpp maps the same reads through the host build of both instantiations; everything a caller can fetch must be identical per read: status, hits
(interval, lower_rev, size, score bits), edit operations and the six event counters.  The host build asserts on every pop that the general step would have
searched backward (the invariant the specialisation rests on), so a frame that breaks it aborts the run.  The models that start in the middle of the read must
be given the general step by the dispatcher."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import presets, synth
from oracle import binding as ob

from parity_util import assert_same_as_oracle, split_reads

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emu", "bwd_step.cpp")
_OUT = os.path.join(_HERE, "emu", "_build", "libbwd_step.so")
_lib = None


def _library():
    """tests/emu/bwd_step.cpp, built on demand with g++ (like emu_util.lib)"""
    global _lib
    if _lib is None:
        csrc = os.path.join(_HERE, "..", "mapad_amd", "csrc")
        deps = [_SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".hip"))]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            tmp = _OUT + f".tmp{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-builtin-log2f", "-fno-builtin-powf",
                                   "-fno-builtin-expf", "-fno-builtin-exp2f", "-fno-builtin-log10f", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                   "-UNDEBUG", "-o", tmp, _SRC])
            os.replace(tmp, _OUT)
        L = C.CDLL(_OUT)
        L.bwd_map_batch.restype = C.POINTER(mb.BatchResultC)
        L.bwd_map_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(mb.Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                    C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.bwd_result_free.restype = None
        L.bwd_result_free.argtypes = [C.POINTER(mb.BatchResultC)]
        _lib = L
    return _lib


def _map(index, params, seqs, quals, offsets, direction, payload_cache):
    """-> (BatchResult, whether the backward-only step ran)"""
    blocks, nb, less, sent = index.device_view()
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    quals = np.ascontiguousarray(quals, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    chosen = C.c_int(-1)
    r = _library().bwd_map_batch(blocks, nb, len(index), less.ctypes.data_as(C.c_void_p), sent.ctypes.data_as(C.c_void_p), C.byref(params),
                                 seqs.ctypes.data_as(C.c_void_p), quals.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), offsets.size - 1,
                                 direction, int(payload_cache), C.byref(chosen))
    return mb.BatchResult(r, _library().bwd_result_free), chosen.value == 1


def _concat(parts):
    seqs = np.concatenate([p[0] for p in parts])
    quals = np.concatenate([p[1] for p in parts])
    lens = np.concatenate([np.diff(p[2].astype(np.int64)) for p in parts])
    offsets = np.zeros(lens.size + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    return seqs, quals, offsets


def _end_indel_reads(g, n, seed):
    """genome pieces of 30-60 bp with one insertion or deletion of 1-2 bases 1-8 positions from the 5' or the 3' end: on both sides of the gap_dist_ends gate (5)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out, lens = [], []
    for _ in range(n):
        L = int(rng.integers(30, 61))
        p = int(rng.integers(0, len(g) - L - 8))
        s = g[p:p + L + 4].copy()
        d = int(rng.integers(1, 9))
        at = d if rng.random() < 0.5 else L - d
        k = int(rng.integers(1, 3))
        s = np.concatenate([s[:at], s[at + k:]]) if rng.random() < 0.5 else np.concatenate([s[:at], acgt[rng.integers(0, 4, k)], s[at:]])
        s = s[:L]
        if rng.random() < 0.5:
            s = synth.revcomp(s)
        out.append(s)
        lens.append(L)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    seqs = np.concatenate(out)
    return seqs, rng.integers(20, 41, seqs.size).astype(np.uint8), offsets


def _batch(g, name, n):
    dmg = dict(f=0.5, t=0.5, d=0.02, s=1.0)
    kw = dict(qual=40) if name == "c2" else dict(qual_range=(20, 40), damage=dmg)
    parts = [synth.reads(g, n, 50, seed=31 + len(name), **kw)]
    if name == "c5_mix":  # the length mix with indels of the C5 line
        parts.append(synth.reads(g, n // 4, 50, seed=77, qual_range=(20, 40), damage=dmg, len_range=(25, 120), indel_frac=0.1))
    parts.append(_end_indel_reads(g, n // 8, seed=5 + len(name)))
    parts.append(synth.reads(g, 60, 50, seed=3, qual_range=(2, 40), len_range=(1, 3)))  # reads of one to three bases
    return _concat(parts)


def _same(a, b, offsets):
    assert a.n_reads == b.n_reads == len(offsets) - 1
    assert np.array_equal(a.status, b.status), "status differs"
    assert np.array_equal(a.hit_begin, b.hit_begin), "hit counts differ"
    for k in ("lower", "lower_rev", "size", "n_ops"):
        assert np.array_equal(a.hits_arr[k], b.hits_arr[k]), k
    assert np.array_equal(a.hits_arr["score"].view(np.uint32), b.hits_arr["score"].view(np.uint32)), "score bits differ"
    assert np.array_equal(a.ops, b.ops), "edit operations differ"
    for k in ("e_search", "e_darray", "n_push", "n_pop", "n_node", "n_hits"):
        assert np.array_equal(a.counters[k], b.counters[k]), f"counter {k} differs"


@pytest.fixture(scope="module")
def genome_and_index():
    g = synth.genome(120_000, seed=4242)
    return g, mapad_amd.Index.build([("chr1", g)])


@pytest.mark.parametrize("payload_cache", [False, True], ids=["lane_parallel_commit", "payload_cache"])
@pytest.mark.parametrize("batch,preset", [("c2", "NO_DAMAGE"), ("c3", "DAMAGE"), ("c5_mix", "DAMAGE"), ("c3", "CONTINUOUS"), ("c3", "DOUBLE_STRANDED"), ("c3", "IGNORE_BQ")])
def test_backward_only_step_equals_general_step(genome_and_index, batch, preset, payload_cache):
    g, idx = genome_and_index
    seqs, quals, offsets = _batch(g, batch, 2400)
    params = mapad_amd.make_params(presets.resolve(getattr(presets, preset)))
    general, ran_bwd = _map(idx, params, seqs, quals, offsets, 0, payload_cache)
    assert not ran_bwd
    special, ran_bwd = _map(idx, params, seqs, quals, offsets, 1, payload_cache)
    assert ran_bwd
    _same(general, special, offsets)
    assert int(general.counters["n_pop"].sum()) > 10 * (len(offsets) - 1)  # the batch did search
    assert int(general.hits_arr["n_ops"].size) > 0
    chosen, ran_bwd = _map(idx, params, seqs, quals, offsets, -1, payload_cache)
    assert ran_bwd, "the production model must get the backward-only step"
    _same(general, chosen, offsets)


def test_backward_only_step_matches_the_oracle(genome_and_index):
    g, idx = genome_and_index
    seqs, quals, offsets = _batch(g, "c5_mix", 400)
    rp = presets.resolve(presets.DAMAGE)
    res, ran_bwd = _map(idx, mapad_amd.make_params(rp), seqs, quals, offsets, 1, False)
    assert ran_bwd
    oidx = ob.OracleIndex.from_bwt(idx.bwt(), "$ACGTX", 128)
    reads, qs = split_reads(seqs, quals, offsets)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
    assert_same_as_oracle(ores, res, offsets)


def test_dispatcher_keeps_the_general_step_for_models_that_start_in_the_middle(genome_and_index):
    g, idx = genome_and_index
    seqs, quals, offsets = synth.reads(g, 300, 50, seed=12, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0), len_range=(35, 70), indel_frac=0.05)
    rp = presets.resolve(presets.VINDIJA)
    params = mapad_amd.make_params(rp)
    chosen, ran_bwd = _map(idx, params, seqs, quals, offsets, -1, False)
    assert not ran_bwd, "VindijaPwm searches both ways: the general step"
    general, _ = _map(idx, params, seqs, quals, offsets, 0, False)
    _same(general, chosen, offsets)
    oidx = ob.OracleIndex.from_bwt(idx.bwt(), "$ACGTX", 128)
    reads, qs = split_reads(seqs, quals, offsets)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
    assert_same_as_oracle(ores, chosen, offsets)
