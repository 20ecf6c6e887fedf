"""What the quality rescaling costs: one process, one GPU, one C4-like batch (48 Mbp genome, 1 M x 50 bp reads with ss damage, the damage
preset).

After a warm-up batch, `--reps` times (default 3) each — everything off, then the damage score alone, then the quality rescaling alone, then off again — a
fresh mapad_map_batch_device + fetch of the same batch followed by mapad_hits_to_coords_gpu (the call `mapad-amd map` makes per chunk), timed on the host.
Every line of output is one measurement: the wall time of the coordinates call, the HIP-event time from records_kernel to the end of text_kernel
(mapad_last_locate_info: the stages run between the two) and the stage's own HIP-event time for that batch — dscore_kernel, which walks the same columns and
is the yardstick (this stage leaves it as it was), or the device-to-device copy of the qualities plus rescale_kernel — and the bytes the stage adds to what
leaves the device per batch.  The expectation is only that the rescaling costs about twice dscore_kernel plus the copy.  Nothing asserts it.
Usage: python profiles/rescale_cost.py [--reads N] [--genome BP] [--reps K]
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
    n, bases = args.reads, int(batch[2][-1])
    print(json.dumps({"setup_s": round(time.time() - t0, 1), "reads": n, "bases": bases, "genome": args.genome}), flush=True)
    ctx = mapad_amd.Context(index, mapad_amd.make_params(presets.resolve(presets.DAMAGE)), 0)
    ctx.set_fetch_d_arrays(False)
    ctx.prepare_lengths([50])

    def one(what, rep):
        t = time.perf_counter()
        ctx.map_batch_device(dev[0], dev[1], dev[2], n, 50)
        res = ctx.fetch()
        t_map = time.perf_counter() - t
        before = ctx.damage_scores(), ctx.quality_rescale()
        co = C.c_void_p()
        t = time.perf_counter()
        rc = L.mapad_hits_to_coords_gpu(ctx.h, res._cptr, 7, C.byref(co))
        t_coords = time.perf_counter() - t
        assert rc == 0, rc
        L.mapad_coords_free(co)
        after = ctx.damage_scores(), ctx.quality_rescale()
        dscore_ms, rescale_ms = (a["kernel_ms"] - b["kernel_ms"] for a, b in zip(after, before))
        line = {"what": what, "rep": rep, "map_fetch_wall_ms": round(t_map * 1e3, 2), "coords_wall_ms": round(t_coords * 1e3, 3),
                "records_to_text_ms": round(ctx.locate_info()[0], 4), "dscore_kernel_ms": round(dscore_ms, 4), "rescale_copy_and_kernel_ms": round(rescale_ms, 4),
                "extra_d2h_bytes": (5 * n if dscore_ms > 0 else 0) + (bases if rescale_ms > 0 else 0)}
        if rescale_ms > 0:
            a, b = after[1], before[1]
            line.update(reads_rescaled=a["reads_rescaled"] - b["reads_rescaled"], candidate_columns=[int(x - y) for x, y in zip(a["candidate_columns"], b["candidate_columns"])],
                        bases_changed=a["bases_changed"] - b["bases_changed"])
        print(json.dumps(line), flush=True)
        res.close()
        return dscore_ms, rescale_ms

    one("warm-up (off)", 0)
    for rep in range(args.reps):
        one("off", rep)
    ctx.set_damage_score(1)
    one("warm-up (damage score)", 0)
    ds = [one("damage score", rep)[0] for rep in range(args.reps)]
    ctx.set_damage_score(0)
    ctx.set_quality_rescale(1)
    one("warm-up (rescale)", 0)
    rs = [one("rescale", rep)[1] for rep in range(args.reps)]
    ctx.set_quality_rescale(0)
    for rep in range(args.reps):
        one("off again", rep)
    print(json.dumps({"dscore_kernel_ms_median": round(float(np.median(ds)), 4), "rescale_copy_and_kernel_ms_median": round(float(np.median(rs)), 4),
                      "rescale_over_dscore": round(float(np.median(rs) / np.median(ds)), 3), "rescaled_bytes_per_batch": bases}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
