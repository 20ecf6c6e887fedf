"""What adapter trimming and read-pair merging cost (DESIGN.md section 4 "Trim and merge"): one process, one GPU, 1 M synthetic pairs of 2 x 100 bases whose
fragment lengths are spread evenly over 25 .. 250 (the TruSeq adapters behind the fragment, random bases behind them, 1 % substitutions).

After a warm-up call, `--reps` times (default 3): mapad_merge_pairs over the pairs in host memory — its wall time, and the HIP-event times of
merge_decide_kernel and merge_write_kernel that the result carries — and mapad_merge_pairs_host over the same pairs on `--threads` host threads (default 16,
through MAPAD_HOST_CPUS).  The yardsticks are the host path and the byte floor: the bytes the two kernels have to move (both mates' bases and qualities in —
the bases twice, once per kernel —, the merged bases and qualities out, the offsets and the per-pair fields) divided by the kernels' time.  Every line of
output is one measurement.  Nothing is asserted.
Usage: python profiles/merge_cost.py [--pairs N] [--reps K] [--threads T]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A1 = np.frombuffer(b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", np.uint8)
A2 = np.frombuffer(b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT", np.uint8)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def synthetic_pairs(n, L, seed):
    rng = np.random.default_rng(seed)
    F = rng.integers(25, 251, n)
    frag = rng.integers(0, 4, (n, 250), dtype=np.uint8)  # codes; the complement of code c is 3 - c
    p = np.arange(L)[None, :]

    def mate(codes_at, adapter):
        inside, in_adapter = p < F[:, None], (p >= F[:, None]) & (p < F[:, None] + len(adapter))
        out = ACGT[rng.integers(0, 4, (n, L), dtype=np.uint8)]
        out = np.where(in_adapter, adapter[np.clip(p - F[:, None], 0, len(adapter) - 1)], out)
        out = np.where(inside, ACGT[codes_at], out)
        flip = rng.random((n, L)) < 0.01
        return np.where(flip, ACGT[rng.integers(0, 4, (n, L), dtype=np.uint8)], out).astype(np.uint8)
    r1 = mate(np.take_along_axis(frag, np.clip(p + 0 * F[:, None], 0, 249), axis=1), A1)
    r2 = mate(3 - np.take_along_axis(frag, np.clip(F[:, None] - 1 - p, 0, 249), axis=1), A2)
    quals = rng.integers(20, 41, (2, n, L), dtype=np.uint8)
    offsets = (np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
    return (r1.ravel(), quals[0].ravel(), offsets, r2.ravel(), quals[1].ravel(), offsets.copy()), F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    os.environ["MAPAD_HOST_CPUS"] = str(args.threads)  # read once, at the host path's first call
    from mapad_amd import binding as mb
    t0 = time.time()
    batch, F = synthetic_pairs(args.pairs, 100, 99)
    n = args.pairs
    print(json.dumps({"setup_s": round(time.time() - t0, 1), "pairs": n, "bases_in": int(batch[0].size + batch[3].size)}), flush=True)
    params = mb.merge_params()
    m = mb.Merger(params)
    dec, wr = [], []
    moved = 0
    for rep in range(-1, args.reps):
        t = time.perf_counter()
        res = m.merge_pairs(*batch)
        wall = time.perf_counter() - t
        bases_in, bases_out = res["counts"]["bases_in"], res["counts"]["bases_out"]
        moved = 3 * bases_in + 2 * bases_out + n * (2 * 16 + 2 * 8 + 13 + 8 + 13)  # decide: bases, offsets in, fields out; scan; write: bases + qualities, offsets, fields in, reads out
        print(json.dumps({"what": "warm-up" if rep < 0 else "gpu", "rep": max(rep, 0), "merge_pairs_wall_ms": round(wall * 1e3, 2), "decide_kernel_ms": round(res["kernel_ms"][0], 4),
                          "write_kernel_ms": round(res["kernel_ms"][1], 4), "merged": int(res["counts"]["class_counts"][0]), "bases_out": int(bases_out),
                          "right_length": int((res["frag_len"] == F).sum())}), flush=True)
        if rep >= 0:
            dec.append(res["kernel_ms"][0])
            wr.append(res["kernel_ms"][1])
    m.close()
    host = []
    for rep in range(args.reps):
        t = time.perf_counter()
        res = mb.merge_pairs_host(params, *batch)
        host.append(time.perf_counter() - t)
        print(json.dumps({"what": "host", "rep": rep, "threads": args.threads, "merge_pairs_host_wall_ms": round(host[-1] * 1e3, 2)}), flush=True)
    k = float(np.median(dec) + np.median(wr))
    print(json.dumps({"decide_kernel_ms_median": round(float(np.median(dec)), 4), "write_kernel_ms_median": round(float(np.median(wr)), 4), "bytes_moved": int(moved),
                      "gb_per_s_over_kernel_time": round(moved / (k * 1e-3) / 1e9, 1) if k > 0 else None, "host_wall_ms_median": round(float(np.median(host)) * 1e3, 2),
                      "host_threads": args.threads}), flush=True)


if __name__ == "__main__":
    main()
