"""What duplicate collapsing costs and what it saves: one process, one GPU, the C2 setting (48 Mbp genome, 1 M x 50 bp reads, no-damage model).

  U = 1 M distinct reads; B = U twice, shuffled (2 M reads).
  depth 1, mapad_map_batch_device + fetch:   U off / U on / B off / B on  -> search ms (mapad_last_kernel_ms), call wall time, grouping us, fan-out us
  depth 2, four batches of B back to back:   on and off                    -> reads/s (a grouping kernel that does not fit beside the running search would show here)
Every setting `--reps` times (default 3), interleaved; every line of output is one measurement.  Usage: python profiles/collapse_cost.py [--reads N] [--genome BP] [--reps K]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mapad_amd  # noqa: E402
from mapad_amd import presets, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=48_000_000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    mapad_amd.lib()
    paths = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln})
    hip = C.CDLL(paths[0] if paths else "libamdhip64.so")

    def to_device(a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 8))) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        return p.value

    t0 = time.time()
    g = synth.genome(args.genome, seed=1234, threads=8)
    index = mapad_amd.Index.build([("chr1", g)], seed=1234, device=0)
    u = synth.reads(g, args.reads, 50, seed=4321, qual=40)
    n = args.reads
    perm = np.random.Generator(np.random.PCG64(1)).permutation(np.concatenate([np.arange(n), np.arange(n)]))
    b_seqs = u[0].reshape(n, 50)[perm].reshape(-1)
    b = (b_seqs, np.full(b_seqs.size, 40, np.uint8), np.arange(0, 50 * 2 * n + 1, 50, dtype=np.uint64))
    batches = {"U": (u, [to_device(a) for a in u]), "B": (b, [to_device(a) for a in b])}
    print(json.dumps({"setup_s": round(time.time() - t0, 1), "reads_U": n, "reads_B": 2 * n, "genome": args.genome}), flush=True)
    params = mapad_amd.make_params(presets.resolve(presets.NO_DAMAGE))

    def context(collapse, depth):
        ctx = mapad_amd.Context(index, params, 0)
        ctx.set_fetch_d_arrays(False)
        ctx.set_collapse_duplicates(collapse)
        ctx.set_pipeline_depth(depth)
        ctx.prepare_lengths([50])
        return ctx

    ctxs = {c: context(c, 1) for c in (False, True)}
    digest = {}
    for rep in range(args.reps + 1):  # (rep 0 warms up: first launches, pool growth)
        for name in ("U", "B"):
            for collapse in (False, True):
                ctx = ctxs[collapse]
                (_, _, offsets), dev = batches[name]
                t = time.perf_counter()
                ctx.map_batch_device(dev[0], dev[1], dev[2], len(offsets) - 1, 50)
                res = ctx.fetch()
                wall = time.perf_counter() - t
                ms = ctx.kernel_ms()
                info = ctx.collapse_info()
                import hashlib
                h = hashlib.sha256()
                for a in (res.hit_begin, res.hits_arr, res.ops, res.status, res.counters):
                    h.update(np.ascontiguousarray(a).tobytes())
                digest.setdefault(name, set()).add(h.hexdigest())
                print(json.dumps({"rep": rep, "batch": name, "collapse": collapse, "darray_order_ms": round(float(ms[0]), 3), "search_ms": round(float(ms[1]), 3), "wall_ms": round(wall * 1e3, 2),
                                  "groups": info[1], "twins": info[2], "pops_executed": info[4], "grouping_us": info[5], "fanout_us": info[6], "n_hits": res.n_hits}), flush=True)
                res.close()
    for c in ctxs.values():
        c.close()
    print(json.dumps({"results_identical_on_off": {k: len(v) == 1 for k, v in digest.items()}}), flush=True)
    (_, _, offsets), dev = batches["B"]
    for rep in range(args.reps + 1):
        for collapse in (False, True):
            ctx = context(collapse, 2)
            for _ in range(2):  # (warm-up of this context's two slots: buffers, first launches)
                ctx.map_batch_device(dev[0], dev[1], dev[2], len(offsets) - 1, 50)
                ctx.fetch().close()
            hip.hipDeviceSynchronize()
            t = time.perf_counter()
            n_hits = 0
            for k in range(4):
                ctx.map_batch_device(dev[0], dev[1], dev[2], len(offsets) - 1, 50)
                if k >= 1:
                    ctx.select_batch(1)
                    r = ctx.fetch(); n_hits += r.n_hits; r.close()
                    ctx.select_batch(0)
            r = ctx.fetch(); n_hits += r.n_hits; r.close()
            wall = time.perf_counter() - t
            print(json.dumps({"rep": rep, "batch": "B x 4, depth 2", "collapse": collapse, "wall_ms": round(wall * 1e3, 1), "reads_per_s": round(4 * 2 * n / wall), "n_hits": n_hits,
                              "grouping_us_last": ctx.collapse_info()[5], "fanout_us_last": ctx.collapse_info()[6]}), flush=True)
            ctx.close()


if __name__ == "__main__":
    main()
