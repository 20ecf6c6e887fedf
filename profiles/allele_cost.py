"""What the allele likelihoods cost: one process, one GPU, one C4-like batch (48 Mbp genome, 1 M x 50 bp reads with ss damage, the damage
preset).

After a warm-up batch, `--reps` times (default 3) each — everything off, then the pileup AND the allele likelihoods on, then off again — a fresh
mapad_map_batch_device + fetch of the same batch followed by mapad_hits_to_coords_gpu (the call `mapad-amd map` makes per chunk), timed on the host.  Every
line of output is one measurement: the search's event times (mapad_last_kernel_ms), the wall time of the coordinates call, the HIP-event time from
records_kernel to the end of text_kernel (mapad_last_locate_info: pileup_kernel and allele_kernel run between the two) and — on — the HIP-event times of
pileup_kernel and of allele_kernel for that batch, from the same run, and their ratio.  The expectation is only that allele_kernel costs a small multiple of
pileup_kernel: five atomics per column where the pileup issues one.  Nothing asserts it.
Usage: python profiles/allele_cost.py [--reads N] [--genome BP] [--reps K]
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
    batch = synth.reads(g, args.reads, 50, seed=4321, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0))
    dev = [to_device(a) for a in batch]
    n = args.reads
    print(json.dumps({"setup_s": round(time.time() - t0, 1), "reads": n, "genome": args.genome}), flush=True)
    ctx = mapad_amd.Context(index, mapad_amd.make_params(presets.resolve(presets.DAMAGE)), 0)
    ctx.set_fetch_d_arrays(False)
    ctx.prepare_lengths([50])

    def one(what, rep):
        t = time.perf_counter()
        ctx.map_batch_device(dev[0], dev[1], dev[2], n, 50)
        res = ctx.fetch()
        t_map = time.perf_counter() - t
        ms = ctx.kernel_ms()
        before = ctx.allele_summary(), ctx.pileup()
        co = C.c_void_p()
        t = time.perf_counter()
        rc = L.mapad_hits_to_coords_gpu(ctx.h, res._cptr, 7, C.byref(co))
        t_coords = time.perf_counter() - t
        assert rc == 0, rc
        L.mapad_coords_free(co)
        after = ctx.allele_summary(), ctx.pileup()
        records_on_ms = ctx.locate_info()[0]
        allele_ms, pileup_ms = (a["accumulate_ms"] - b["accumulate_ms"] for a, b in zip(after, before))
        print(json.dumps({"what": what, "rep": rep, "map_fetch_wall_ms": round(t_map * 1e3, 2), "darray_order_ms": round(float(ms[0]), 3), "search_ms": round(float(ms[1]), 3),
                          "coords_wall_ms": round(t_coords * 1e3, 3), "records_kernel_on_ms": round(records_on_ms, 4), "allele_kernel_ms": round(allele_ms, 4),
                          "pileup_kernel_ms": round(pileup_ms, 4), "allele_over_pileup": round(allele_ms / pileup_ms, 3) if pileup_ms > 0 else None,
                          "allele_batches": after[0]["batches"], "columns_counted": after[0]["columns_counted"] - before[0]["columns_counted"],
                          "pileup_columns_counted": after[1]["columns_counted"] - before[1]["columns_counted"], "summary_ms": round(after[0]["summary_ms"], 4),
                          "sites_called": sum(c["sites_called"] for c in after[0]["contigs"])}), flush=True)
        res.close()

    one("warm-up (off)", 0)
    for rep in range(args.reps):
        one("off", rep)
    ctx.set_pileup(1)
    ctx.set_allele_likelihoods(1)
    one("warm-up (on)", 0)
    for rep in range(args.reps):
        one("on", rep)
    ctx.set_pileup(0)
    ctx.set_allele_likelihoods(0)
    for rep in range(args.reps):
        one("off again", rep)
    ctx.close()


if __name__ == "__main__":
    main()
