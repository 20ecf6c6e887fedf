"""What the SNP panel costs ("SNP panel"): one process, one GPU, one C4-like batch (48 Mbp genome, 1 M x 50 bp reads with ss damage, the damage
preset), mapped once.

Per panel — one row per 2 500 bp (the density of a capture panel), one row per 50 bp (every read holds a slot), and 1.2 M rows (one per 40 bp: the size of the
1240K panel, for the call kernel) — the pileup and the panel are switched on, and `--reps` times (default 3) both tables are reset and the resident batch is
converted again with mapad_hits_to_coords_gpu (the call `mapad-amd map` makes per chunk): pileup_kernel and panel_kernel run over the same batch in the same
call.  Every line of output is one measurement: the HIP-event times of the two kernels for that batch and their ratio, the panel's counters, then the HIP-event
time of panel_call_kernel over all rows (the summary) and the wall times of the calls and counts read-outs.  The design claim is only that the sparse panel
costs clearly less than the pileup, because nearly every read ends behind the search.  Nothing asserts it.
Usage: python profiles/panel_cost.py [--reads N] [--genome BP] [--reps K]
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
    t0 = time.time()
    g = synth.genome(args.genome, seed=1234, threads=8)
    index = mapad_amd.Index.build([("chr1", g)], seed=1234, device=0)
    batch = synth.reads(g, args.reads, 50, seed=4321, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0))
    print(json.dumps({"setup_s": round(time.time() - t0, 1), "reads": args.reads, "genome": args.genome}), flush=True)
    ctx = mapad_amd.Context(index, mapad_amd.make_params(presets.resolve(presets.DAMAGE)), 0)
    ctx.set_fetch_d_arrays(False)
    res = ctx.map_batch(*batch)
    letters = np.frombuffer(b"ACGT", np.uint8)
    code = np.zeros(256, np.int64)
    code[letters] = np.arange(4)

    def convert():
        co = C.c_void_p()
        t = time.perf_counter()
        rc = L.mapad_hits_to_coords_gpu(ctx.h, res._cptr, 7, C.byref(co))
        wall = time.perf_counter() - t
        assert rc == 0, rc
        L.mapad_coords_free(co)
        return wall

    ctx.set_pileup(1)
    rule = dict(call="random", min_depth=1, transitions="single_strand", seed=1)
    for name, every in (("one row per 2500 bp", 2500), ("one row per 50 bp", 50), ("1.2 M rows (one per 40 bp)", 40)):
        pos0 = np.arange(every // 2, args.genome, every, dtype=np.uint64)
        ref = g[pos0.astype(np.int64)]
        alt = letters[(code[ref] + 2) & 3]  # the transition partner
        ctx.set_snp_panel(1, np.zeros(len(pos0), np.int32), pos0, ref, alt)
        convert()  # warm-up
        for rep in range(args.reps):
            ctx.pileup_reset()
            ctx.snp_panel_reset()
            wall = convert()
            pan, pil = ctx.snp_panel(rule), ctx.pileup()
            t = time.perf_counter()
            calls = ctx.snp_panel_calls(0, len(pos0), rule)
            t_calls = time.perf_counter() - t
            t = time.perf_counter()
            ctx.snp_panel_counts(0, len(pos0))
            t_counts = time.perf_counter() - t
            print(json.dumps({"panel": name, "rows": len(pos0), "rep": rep, "coords_wall_ms": round(wall * 1e3, 3), "panel_kernel_ms": round(pan["accumulate_ms"], 4),
                              "pileup_kernel_ms": round(pil["accumulate_ms"], 4), "panel_over_pileup": round(pan["accumulate_ms"] / pil["accumulate_ms"], 3),
                              "reads": pan["reads"], "reads_on_panel": pan["reads_on_panel"], "columns_counted": pan["columns_counted"],
                              "pileup_columns_counted": pil["columns_counted"], "panel_call_kernel_ms": round(pan["summary_ms"], 4), "rows_called": pan["rows_called"],
                              "calls_readout_wall_ms": round(t_calls * 1e3, 3), "counts_readout_wall_ms": round(t_counts * 1e3, 3),
                              "called_in_readout": int((calls != ord("9")).sum())}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
