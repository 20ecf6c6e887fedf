"""What the diploid genotype likelihoods cost: one GPU, one C4-like batch (48 Mbp genome, 1 M x 50 bp reads with ss damage, the damage
preset).

The measuring runs in a child process of its own under `timeout -k 10 --limit` (default 900 s): this process never touches the GPU and passes the child's exit
status on.  In the child, after a warm-up batch, `--reps` times (default 3) with the pileup, the allele likelihoods AND the genotype likelihoods on: a fresh
mapad_map_batch_device + fetch of the same batch followed by mapad_hits_to_coords_gpu (the call `mapad-amd map` makes per chunk).  Every line of output is one
measurement: the HIP-event times of pileup_kernel, allele_kernel and genotype_kernel for that batch, from the same run, the ratio genotype / allele, and the
HIP-event time of one genotype_call_kernel pass over the genome (a summary).  The expectation from the code is only that genotype_kernel costs about what
allele_kernel costs: six atomics and a 16-byte load per column against five and a 16-byte load.  Nothing asserts it.
Usage: python profiles/genotype_cost.py [--reads N] [--genome BP] [--reps K] [--limit SECONDS]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(args):
    import numpy as np

    import mapad_amd
    from mapad_amd import presets, synth

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
    dev = [to_device(a) for a in batch]  # seqs, quals, offsets: offsets has reads + 1 entries, the batch below names `reads` reads
    n = len(batch[2]) - 1
    assert n == args.reads
    print(json.dumps({"setup_s": round(time.time() - t0, 1), "reads": n, "genome": args.genome}), flush=True)
    ctx = mapad_amd.Context(index, mapad_amd.make_params(presets.resolve(presets.DAMAGE)), 0)
    ctx.set_fetch_d_arrays(False)
    ctx.prepare_lengths([50])
    ctx.set_pileup(1)
    ctx.set_allele_likelihoods(1)
    ctx.set_genotype_likelihoods(True)

    def one(what, rep):
        ctx.map_batch_device(dev[0], dev[1], dev[2], n, 50)
        res = ctx.fetch()
        before = ctx.genotype_summary(1, 3.0, 10.0), ctx.allele_summary(), ctx.pileup()
        co = C.c_void_p()
        t = time.perf_counter()
        rc = L.mapad_hits_to_coords_gpu(ctx.h, res._cptr, 7, C.byref(co))
        t_coords = time.perf_counter() - t
        assert rc == 0, rc
        L.mapad_coords_free(co)
        after = ctx.genotype_summary(1, 3.0, 10.0), ctx.allele_summary(), ctx.pileup()
        gt_ms, al_ms, pil_ms = (a["accumulate_ms"] - b["accumulate_ms"] for a, b in zip(after, before))
        print(json.dumps({"what": what, "rep": rep, "coords_wall_ms": round(t_coords * 1e3, 3), "genotype_kernel_ms": round(gt_ms, 4), "allele_kernel_ms": round(al_ms, 4),
                          "pileup_kernel_ms": round(pil_ms, 4), "genotype_over_allele": round(gt_ms / al_ms, 3) if al_ms > 0 else None,
                          "genotype_batches": after[0]["batches"], "columns_counted": after[1]["columns_counted"] - before[1]["columns_counted"],
                          "genotype_call_pass_ms": round(after[0]["summary_ms"], 4), "allele_call_pass_ms": round(after[1]["summary_ms"], 4),
                          "sites_called": sum(c["sites_called"] for c in after[0]["contigs"]), "het_called": sum(sum(c["called"][4:]) for c in after[0]["contigs"])}), flush=True)
        res.close()

    one("warm-up", 0)
    for rep in range(args.reps):
        one("on", rep)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=48_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--run", action="store_true", help="measure in this process (what the parent starts under its time limit)")
    args = ap.parse_args()
    if args.run:
        return measure(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--run", "--reads", str(args.reads), "--genome", str(args.genome), "--reps", str(args.reps)]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
