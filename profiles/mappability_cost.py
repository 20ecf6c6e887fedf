"""What the mappability stage costs (DESIGN.md sections 4 and 5): one process, one GPU, one of the bench's synthetic genomes (default 48 Mbp, seed 1234, one
contig; the size is in the output).

For k = 35 and e = 0, then e = 1: after one warm-up call, `--reps` calls (default 3) of mapad_ctx_mappability over the whole contig, counts and cover fetched.
Every line of output is one measurement: the wall time of the call on the host (uploads, the three kernels' tiles, downloads), the HIP-event time of the count
kernels alone (mapad_last_mappability_info), starts per second by either, and the rank queries per start (two per extension step).  Beside them the same two
cases through mapad_mappability_host on this process's CPUs (mapad_host_cpus), over a window of `--host_starts` starts in the middle of the contig (default
4 M: the host path is slow, the window is stated in the output), and whether the window's bytes equal the device's.
Usage: python profiles/mappability_cost.py [--genome BP] [--reps K] [--host_starts N] [--k 35]
"""
import argparse
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
    ap.add_argument("--genome", type=int, default=48_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host_starts", type=int, default=4_000_000)
    ap.add_argument("--k", type=int, default=35)
    args = ap.parse_args()
    t0 = time.time()
    g = synth.genome(args.genome, seed=1234, threads=8)
    index = mapad_amd.Index.build([("chr1", g)], seed=1234, device=0)
    ctx = mapad_amd.Context(index, mapad_amd.make_params(presets.resolve(presets.DAMAGE)), 0)
    cpus = int(mapad_amd.lib().mapad_host_cpus())
    print(json.dumps({"setup_s": round(time.time() - t0, 1), "genome": args.genome, "k": args.k, "host_cpus": cpus}), flush=True)
    n = int(g.size)
    w_n = min(args.host_starts, n)
    w_from = (n - w_n) // 2
    for e in (0, 1):
        device = None
        for rep in range(-1, args.reps):
            t = time.perf_counter()
            device = ctx.mappability(0, g, k=args.k, e=e)
            wall = time.perf_counter() - t
            ms, starts, steps = ctx.mappability_info()
            print(json.dumps({"what": "device warm-up" if rep < 0 else "device", "e": e, "rep": max(rep, 0), "starts": starts, "call_wall_ms": round(wall * 1e3, 2),
                              "count_kernel_ms": round(ms, 3), "starts_per_s_kernel": round(starts / (ms * 1e-3)), "starts_per_s_call": round(starts / wall),
                              "rank_queries_per_start": round(2 * steps / starts, 2), "unique_fraction": round(float((device[0] == 1).mean()), 4)}), flush=True)
        t = time.perf_counter()
        hc, hv = mapad_amd.mappability_host(index, 0, g, start=w_from, n=w_n, k=args.k, e=e)
        wall = time.perf_counter() - t
        same = hc.tobytes() == device[0][w_from:w_from + w_n].tobytes() and hv.tobytes() == device[1][w_from:w_from + w_n].tobytes()
        print(json.dumps({"what": "host", "e": e, "cpus": cpus, "window_from": w_from, "starts": w_n, "wall_ms": round(wall * 1e3, 1), "starts_per_s": round(w_n / wall),
                          "equals_device": bool(same)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
