"""The host half of the host tail (csrc/host_tail.hpp) without a GPU: tests/emu/tail_ring_selftest.cpp — tail_start's dispatcher, TailWorkers, tail_map_read,
tail_finish and tail_cancel are the product's, producer threads play the kernel (give_to_host's claim rule restated, `ready = gen` published with release order).
The program runs as a child process of its own, built plainly, under ThreadSanitizer and under AddressSanitizer + UBSan; nothing of it is loaded into Python."""
import os
import struct
import subprocess

import numpy as np

import mapad_amd
from mapad_amd import synth
from oracle import binding as ob

from kat_util import resolve_params
from parity_util import DAMAGE, split_reads

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emu", "tail_ring_selftest.cpp")
# (the flags of emu_util.tail_bench_lib: the search's arithmetic must be the product's)
_FLAGS = ["-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-fno-builtin-log2f", "-fno-builtin-powf", "-fno-builtin-expf", "-fno-builtin-exp2f",
          "-fno-builtin-log10f", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
BUILDS = {"plain": ["-O2"], "tsan": ["-O1", "-fsanitize=thread"], "asan_ubsan": ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def write_input(path, pidx, params, seqs, quals, offsets, want_pops):
    """magic, n_blocks, n, less[8], sentinel[2], sizeof(mapad_params_t), n_reads, bases | rank blocks | parameters | offsets | bases | qualities | the oracle's pops"""
    _, nb, less, sent = pidx.device_view()
    blocks = pidx.blocks()
    with open(path, "wb") as f:
        f.write(struct.pack("<16Q", 0x4C49415444415041, int(nb), len(pidx), *[int(x) for x in less], *[int(x) for x in sent], len(bytes(params)), len(offsets) - 1, len(seqs)))
        for a, t in ((blocks, np.uint64), (None, None), (offsets, np.uint64), (seqs, np.uint8), (quals, np.uint8), (want_pops, np.uint64)):
            f.write(bytes(params) if a is None else np.ascontiguousarray(a, dtype=t).tobytes())


def selftest_input(path):
    g = synth.genome(80_000, seed=21)
    seqs, quals, offsets = synth.reads(g, 160, 50, seed=12, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0), len_range=(35, 100), indel_frac=0.05)
    rp = dict(resolve_params(DAMAGE), stack_limit=20_000, edit_tree_limit=100_000)  # a worker's arena: 2 MB of heap, 4 MB of nodes
    pidx = mapad_amd.Index.build([("chr1", g)])
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    reads, qs = split_reads(seqs, quals, offsets)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8)
    write_input(path, pidx, mapad_amd.make_params(rp), seqs, quals, offsets, ores.counters[:, 3])
    return ores


def build_all(outdir, src=_SRC):
    """the three builds side by side -> {name: executable}"""
    procs = {name: subprocess.Popen(["g++", *flags, *_FLAGS, "-o", os.path.join(outdir, "tail_ring_selftest." + name), src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for name, flags in BUILDS.items()}
    for name, p in procs.items():
        out, _ = p.communicate()
        assert p.returncode == 0, f"{name}: {out[-4000:]}"
    return {name: os.path.join(outdir, "tail_ring_selftest." + name) for name in BUILDS}


def test_ring_dispatcher_workers_finish_and_cancel_under_sanitizers(tmp_path):
    """Every record's result equals a direct tail_search of the same read (whose pops equal the oracle's) with done == dispatched == count; under a backlog limit L
    the records claimed and not yet picked up never exceed L, and L = 0 admits nobody; one ring over launches of 300, 10, 300, 10 and 250 records hands over exactly
    each launch's own; a ring cursor beyond the ring is clamped; tail_cancel with tasks queued and running returns with done == dispatched and nobody touches the
    (freed) ring afterwards; with two launches alive the backlog word of each shows the tasks of both.  No sanitizer has anything to report."""
    inp = str(tmp_path / "tail_input.bin")
    ores = selftest_input(inp)
    pops = ores.counters[:, 3]
    assert int((pops > 1000).sum()) >= 10 and int(pops.max()) > 10_000  # searches long enough for tasks to queue behind four workers
    exes = build_all(str(tmp_path))
    env = dict(os.environ, MAPAD_TAIL_THREADS="4", TSAN_OPTIONS="halt_on_error=0 exitcode=66", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    runs = {name: subprocess.Popen([exe, inp, "240"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for name, exe in exes.items()}
    for name, p in runs.items():
        out, _ = p.communicate(timeout=300)
        assert p.returncode == 0 and "tail ring selftest ok" in out, f"{name} (exit {p.returncode}):\n{out[-6000:]}"
        assert "Sanitizer" not in out and "runtime error" not in out, f"{name}:\n{out[-6000:]}"
