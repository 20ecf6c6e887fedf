"""What the read clean-up costs (DESIGN.md section 4 "Clean"): one process, one GPU, 1 M synthetic reads of 100 bases with all four ops on — random bases with
qualities of 3 .. 40; every fifth read ends in a poly-G tail of 10 .. 40 bases, every seventh has 1 .. 4 N in front and as many bases of quality 2 behind, every
fiftieth is a repeat of period 1 .. 4.

After a warm-up call, `--reps` times (default 3): mapad_clean_reads over the reads in host memory — its wall time, and the HIP-event times of clean_decide_kernel
and clean_write_kernel that the result carries — and mapad_clean_reads_host over the same reads on `--threads` host threads (default 16, through
MAPAD_HOST_CPUS).  The yardsticks are the host path and the byte floor: the bytes the two kernels have to move (decide: bases, qualities and offsets in, the
per-read fields out; write: the kept bases and qualities in and out, offsets and fields in) divided by the kernels' time.  Every line of output is one
measurement.  Nothing is asserted.
Usage: python profiles/clean_cost.py [--reads N] [--reps K] [--threads T]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACGT = np.frombuffer(b"ACGT", np.uint8)


def synthetic_reads(n, L, seed):
    rng = np.random.default_rng(seed)
    r = ACGT[rng.integers(0, 4, (n, L), dtype=np.uint8)]
    q = rng.integers(3, 41, (n, L), dtype=np.uint8)
    p = np.arange(L)[None, :]
    i = np.arange(n)
    tail = np.where(i % 5 == 0, rng.integers(10, 41, n), 0)[:, None]
    r = np.where(p >= L - tail, np.uint8(ord("G")), r)
    ends = np.where(i % 7 == 0, rng.integers(1, 5, n), 0)[:, None]
    r = np.where(p < ends, np.uint8(ord("N")), r)
    q = np.where((p >= L - tail - ends) & (p < L - tail), np.uint8(2), q)
    period = rng.integers(1, 5, n)[:, None]
    unit = ACGT[rng.integers(0, 4, (n, 4), dtype=np.uint8)]
    r = np.where((i % 50 == 0)[:, None], np.take_along_axis(unit, p % period, axis=1), r)
    offsets = (np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
    return np.ascontiguousarray(r, np.uint8).ravel(), np.ascontiguousarray(q, np.uint8).ravel(), offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    os.environ["MAPAD_HOST_CPUS"] = str(args.threads)  # read once, at the host path's first call
    from mapad_amd import binding as mb
    t0 = time.time()
    batch = synthetic_reads(args.reads, 100, 99)
    n = args.reads
    print(json.dumps({"setup_s": round(time.time() - t0, 1), "reads": n, "bases_in": int(batch[0].size)}), flush=True)
    params = mb.clean_params(15, max_dust=70)
    c = mb.Cleaner(params)
    dec, wr = [], []
    moved_decide = moved_write = 0
    for rep in range(-1, args.reps):
        t = time.perf_counter()
        res = c.clean_reads(*batch)
        wall = time.perf_counter() - t
        k = res["counts"]
        moved_decide = 2 * k["bases_in"] + n * (8 + 13)     # bases, qualities, offsets in; class, three trims, dust, length out
        moved_write = 4 * k["bases_out"] + n * (8 + 8 + 13)  # the kept bases and qualities in and out; both offsets and the fields in
        print(json.dumps({"what": "warm-up" if rep < 0 else "gpu", "rep": max(rep, 0), "clean_reads_wall_ms": round(wall * 1e3, 2), "decide_kernel_ms": round(res["kernel_ms"][0], 4),
                          "write_kernel_ms": round(res["kernel_ms"][1], 4), "classes": [int(v) for v in k["class_counts"]], "bases_out": int(k["bases_out"]),
                          "bases_poly": int(k["bases_poly"]), "bases_trim5": int(k["bases_trim5"]), "bases_trim3": int(k["bases_trim3"])}), flush=True)
        if rep >= 0:
            dec.append(res["kernel_ms"][0])
            wr.append(res["kernel_ms"][1])
    c.close()
    host = []
    same = None
    for rep in range(args.reps):
        t = time.perf_counter()
        h = mb.clean_reads_host(params, *batch)
        host.append(time.perf_counter() - t)
        same = all(np.array_equal(h[f], res[f]) for f in ("cls", "trim5", "trim3", "poly_len", "dust", "offsets", "seqs", "quals"))
        print(json.dumps({"what": "host", "rep": rep, "threads": args.threads, "clean_reads_host_wall_ms": round(host[-1] * 1e3, 2), "equals_device": bool(same)}), flush=True)
    d, w = float(np.median(dec)), float(np.median(wr))
    print(json.dumps({"decide_kernel_ms_median": round(d, 4), "write_kernel_ms_median": round(w, 4), "decide_reads_per_s": round(n / (d * 1e-3)) if d > 0 else None,
                      "write_reads_per_s": round(n / (w * 1e-3)) if w > 0 else None, "decide_bytes": int(moved_decide), "write_bytes": int(moved_write),
                      "decide_gb_per_s": round(moved_decide / (d * 1e-3) / 1e9, 1) if d > 0 else None, "write_gb_per_s": round(moved_write / (w * 1e-3) / 1e9, 1) if w > 0 else None,
                      "host_wall_ms_median": round(float(np.median(host)) * 1e3, 2), "host_threads": args.threads}), flush=True)


if __name__ == "__main__":
    main()
