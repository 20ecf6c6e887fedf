"""The backward-only search kernel (search_kernel<.., BWD = true>, the default for the simple_adna model) against the general kernel on the GPU.

Each batch is mapped by two child processes, one with the default dispatch and one with MAPAD_GENERAL_DIRECTION=1 (the switch is read when a context is created;
separate processes keep the two runs apart the way test_gpu_parity.py keeps its library flavours apart).  Everything a caller can fetch must be byte-identical:
hit offsets, hit records, edit operations, status, event counters.  One oracle comparison pins the pair, so that the two cannot be wrong together."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import mapad_amd
from mapad_amd import presets, synth
from oracle import binding as ob

from parity_util import assert_same_as_oracle, split_reads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)

_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import mapad_amd
from mapad_amd import presets
import test_gpu_bwd as t
name, out = sys.argv[2], sys.argv[3]
g, seqs, quals, offsets, preset = t.batch(name)
idx = mapad_amd.Index.build([("chr1", g)])
ctx = mapad_amd.Context(idx, mapad_amd.make_params(presets.resolve(getattr(presets, preset))), 0)
try:
    r = ctx.map_batch(seqs, quals, offsets)
    np.savez(out, hit_begin=np.asarray(r.hit_begin), hits=np.frombuffer(np.ascontiguousarray(r.hits_arr).tobytes(), np.uint8), ops=np.asarray(r.ops),
             status=np.asarray(r.status), counters=np.frombuffer(np.ascontiguousarray(r.counters).tobytes(), np.uint8))
finally:
    ctx.close()
"""


def batch(name):
    """-> (genome, seqs, quals, offsets, preset name): >= 100 K reads in the style of the C2, C3 and C5-mix benchmark lines (seeded: both children build the same)"""
    g = synth.genome(2_000_000, seed=606)
    if name == "c2":
        return (g,) + synth.reads(g, 120_000, 50, seed=61, qual=40) + ("NO_DAMAGE",)
    if name == "c3":
        return (g,) + synth.reads(g, 120_000, 50, seed=62, qual_range=(20, 40), damage=DMG) + ("DAMAGE",)
    a = synth.reads(g, 100_000, 50, seed=63, qual_range=(20, 40), damage=DMG)
    b = synth.reads(g, 4_000, 50, seed=64, qual_range=(20, 40), damage=DMG, len_range=(25, 120), indel_frac=0.1)
    lens = np.concatenate([np.diff(a[2].astype(np.int64)), np.diff(b[2].astype(np.int64))])
    offsets = np.zeros(lens.size + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    return g, np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), offsets, "DAMAGE"


def _child(name, out, general):
    env = {k: v for k, v in os.environ.items() if k != "MAPAD_GENERAL_DIRECTION"}
    if general:
        env["MAPAD_GENERAL_DIRECTION"] = "1"
    pr = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name, out], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert pr.returncode == 0, pr.stdout[-3000:]
    return np.load(out)


@pytest.mark.parametrize("name", ["c2", "c3", "c5_mix"])
def test_default_dispatch_and_general_direction_fetch_the_same_bytes(name):
    with tempfile.TemporaryDirectory() as d:
        a = _child(name, os.path.join(d, "bwd.npz"), general=False)
        b = _child(name, os.path.join(d, "general.npz"), general=True)
        assert a["status"].size >= 100_000
        assert int(np.asarray(a["hit_begin"])[-1]) > a["status"].size // 2  # most reads map: the comparison is not of empty results
        for k in ("hit_begin", "hits", "ops", "status", "counters"):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{name}: {k} differs between the two kernels"


@pytest.mark.parametrize("general", [False, True], ids=["backward_only", "general_direction"])
def test_both_kernels_match_the_oracle(general, monkeypatch):
    if general:
        monkeypatch.setenv("MAPAD_GENERAL_DIRECTION", "1")
    else:
        monkeypatch.delenv("MAPAD_GENERAL_DIRECTION", raising=False)
    g = synth.genome(300_000, seed=99)
    seqs, quals, offsets = synth.reads(g, 1500, 50, seed=17, qual_range=(20, 40), damage=DMG, len_range=(20, 100), indel_frac=0.1)
    rp = presets.resolve(presets.DAMAGE)
    pidx = mapad_amd.Index.build([("chr1", g)])
    ctx = mapad_amd.Context(pidx, mapad_amd.make_params(rp), 0)
    try:
        res = ctx.map_batch(seqs, quals, offsets)
    finally:
        ctx.close()
    oidx = ob.OracleIndex.from_bwt(pidx.bwt(), "$ACGTX", 128)
    reads, qs = split_reads(seqs, quals, offsets)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
    assert_same_as_oracle(ores, res, offsets)
