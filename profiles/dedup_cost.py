"""What marking PCR duplicates costs: one process, one GPU, one C4-sized batch (48 Mbp genome, 1 M x 50 bp reads with ss damage, the damage
preset; a fifth of the reads drawn twice).

After a warm-up batch, `--reps` times (default 3) each, the mode off and then on, a fresh mapad_map_batch_device + fetch of the same batch followed by
mapad_hits_to_coords_gpu (the call `mapad-amd map` makes per chunk), timed on the host.  Every line of output is one measurement: the search's event times
(mapad_last_kernel_ms), the event time from records_kernel to the end of the post-search kernels (mapad_last_locate_info: records_kernel alone with the mode
off), the wall time of the coordinates call, and — on — the event time of dedup_insert_kernel + dedup_mark_kernel for that batch (mark_ms) and that of
dedup_hist_kernel (summary_ms).  The last lines time one growth: the same batch marked again on top of a table that is full to its limit, so that the call
allocates a table of twice the size and runs dedup_rehash_kernel over every slot (wall time of the call against the calls before it).
Usage: python profiles/dedup_cost.py [--reads N] [--genome BP] [--reps K]
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
    L = mapad_amd.lib()
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
    drawn = synth.reads(g, args.reads - args.reads // 5, 50, seed=4321, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0))
    rng = np.random.Generator(np.random.PCG64(99))
    pick = rng.permutation(np.concatenate([np.arange(args.reads - args.reads // 5), rng.integers(0, args.reads - args.reads // 5, args.reads // 5)]))
    # (all reads are 50 bases; the offsets are those of all args.reads reads, not of the reads drawn: a shorter array is read beyond its end on the device)
    batch = (drawn[0].reshape(-1, 50)[pick].reshape(-1), drawn[1].reshape(-1, 50)[pick].reshape(-1), np.arange(len(pick) + 1, dtype=np.uint64) * np.uint64(50))
    dev = [to_device(a) for a in batch]
    n = args.reads
    print(json.dumps({"setup_s": round(time.time() - t0, 1), "reads": n, "genome": args.genome}), flush=True)
    ctx = mapad_amd.Context(index, mapad_amd.make_params(presets.resolve(presets.DAMAGE)), 0)
    ctx.set_fetch_d_arrays(False)
    ctx.prepare_lengths([50])

    def one(what, rep, on, reset=True):
        t = time.perf_counter()
        ctx.map_batch_device(dev[0], dev[1], dev[2], n, 50)
        res = ctx.fetch()
        t_map = time.perf_counter() - t
        ms = ctx.kernel_ms()
        if on and reset:
            ctx.duplicates_reset()  # one batch per measurement in the table
        before = ctx.duplicates() if on else None
        co = C.c_void_p()
        t = time.perf_counter()
        rc = L.mapad_hits_to_coords_gpu(ctx.h, res._cptr, 7, C.byref(co))
        t_coords = time.perf_counter() - t
        assert rc == 0, rc
        L.mapad_coords_free(co)
        line = {"what": what, "rep": rep, "map_fetch_wall_ms": round(t_map * 1e3, 2), "darray_order_ms": round(float(ms[0]), 3), "search_ms": round(float(ms[1]), 3),
                "post_search_event_ms": round(ctx.locate_info()[0], 4), "coords_wall_ms": round(t_coords * 1e3, 3)}
        if on:
            t = time.perf_counter()
            d = ctx.duplicates()
            t_sum = time.perf_counter() - t
            line.update({"mark_ms": round(d["mark_ms"] - before["mark_ms"], 4), "summary_ms": round(d["summary_ms"], 4), "summary_wall_ms": round(t_sum * 1e3, 3),
                         "reads_eligible": d["reads_eligible"], "duplicates": d["duplicates"], "fragments": d["fragments"], "slots": d["slots"], "grows": d["grows"],
                         "batches": d["batches"]})
        print(json.dumps(line), flush=True)
        res.close()

    one("warm-up (off)", 0, False)
    for rep in range(args.reps):
        one("off", rep, False)
    t = time.perf_counter()
    ctx.set_mark_duplicates(1)
    print(json.dumps({"what": "switch-on", "wall_ms": round((time.perf_counter() - t) * 1e3, 3)}), flush=True)
    one("warm-up (on)", 0, True)
    for rep in range(args.reps):
        one("on", rep, True)
    # one growth: the table is sized for one batch of new keys; the same batch again asks for room for as many more, although it brings none
    one("on, the call grows the table (rehash)", 0, True, reset=False)
    one("on, the grown table", 0, True, reset=False)
    ctx.set_mark_duplicates(0)
    for rep in range(args.reps):
        one("off again", rep, False)
    ctx.close()


if __name__ == "__main__":
    main()
