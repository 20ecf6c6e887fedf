"""What the track build of `mapad_ctx_accumulate_alignments` costs: HIP-event time of align_count_kernel, the scan and align_build_kernel over one batch of
1 M x 50 bp alignments (no stage switched on), on the 400 kbp two-contig world of the tests — the build does not look at the index beyond its contig table.
Half the reads carry `50M` with MD `24C25`, half `20M1D30M` with MD `20^A30`; every other read is on the reverse strand.  One warm-up call, then three timed ones.
Prints one JSON line.  Run on an MI355X: python profiles/analyse_cost.py [n_reads]"""
import json
import os
import sys
import time

import numpy as np

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."), os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests")]

import mapad_amd  # noqa: E402
from mapad_amd import binding as mb  # noqa: E402

import panel_util as pn  # noqa: E402
from kat_util import resolve_params  # noqa: E402
from parity_util import DAMAGE  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    L = 50
    g = pn.world_genome()
    idx = mapad_amd.Index.build([("c1", g[:pn.SPLIT]), ("c2", g[pn.SPLIT:])])
    rng = np.random.default_rng(1)
    deleted = (np.arange(n) & 1).astype(bool)
    alns = np.zeros(n, mb.ALIGNMENT_DTYPE)
    alns["tid"] = rng.integers(0, 2, n)
    alns["pos0"] = rng.integers(0, min(pn.LENGTHS) - 60, n)
    alns["flags"] = np.where((np.arange(n) >> 1) & 1, 0x10, 0)
    alns["mapq"], alns["x0"], alns["as_score"] = 37, 1, -1.0
    alns["cigar_off"] = np.where(deleted, 1, 0)       # word 0: 50M; words 1..3: 20M 1D 30M
    alns["n_cigar"] = np.where(deleted, 3, 1)
    alns["md_off"] = np.where(deleted, 5, 0)          # bytes 0..4: 24C25; bytes 5..10: 20^A30
    alns["md_len"] = np.where(deleted, 6, 5)
    cigar = np.array([50 << 4, 20 << 4, 1 << 4 | 2, 30 << 4], np.uint32)
    md = np.frombuffer(b"24C2520^A30", np.uint8)
    seqs = rng.choice(np.frombuffer(b"ACGT", np.uint8), n * L)
    quals = np.full(n * L, 35, np.uint8)
    offsets = np.arange(n + 1, dtype=np.uint64) * L
    ctx = mapad_amd.Context(idx, mapad_amd.make_params(resolve_params(DAMAGE)), 0)
    ms, wall = [], []
    try:
        for k in range(4):
            t0 = time.perf_counter()
            out = ctx.accumulate_alignments(seqs, quals, offsets, alns, cigar, md)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(out["build_ms"])
            assert out["class_counts"]["ok"] == n, out["class_counts"]
    finally:
        ctx.close()
    print(json.dumps({"n_reads": n, "read_len": L, "build_ms": [round(x, 3) for x in ms[1:]], "reads_per_s": [round(n / (x * 1e-3)) for x in ms[1:]],
                      "call_wall_ms": [round(x, 1) for x in wall[1:]], "warmup_build_ms": round(ms[0], 3)}))


if __name__ == "__main__":
    main()
