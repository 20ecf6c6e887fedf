"""bench.py on the GPU (run with -m gpu on an MI355X): a plain run prints the headline line and nothing beyond it, --steps sets the number of
timed steps, --dump-outputs writes the same arrays for the same arguments, and --full adds the roofline, tail and parity sample."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--config", "c1", "--warmup", "1"]


def _bench(args, timeout=600):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        e.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=e, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_repeatable_dump(tmp_path):
    a = _bench(SMALL + ["--steps", "3", "--dump-outputs", str(tmp_path / "a")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in a
    assert a["steps"] == 3 and a["value"] > 0 and a["ms_per_step"] > 0
    assert abs(a["value"] - a["config"]["reads_per_gpu"] * 1e3 / a["ms_per_step"]) <= 0.02 * a["value"]  # (ms_per_step is rounded to 1 us)
    assert "roofline" not in a and "cpu_baseline" not in a and "secondary" not in a
    names = sorted(a["dump_outputs"]["arrays"])
    assert names and sorted(f[:-4] for f in os.listdir(tmp_path / "a")) == names
    b = _bench(SMALL + ["--steps", "2", "--dump-outputs", str(tmp_path / "b")])
    assert b["steps"] == 2
    total = 0
    for name in names:
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), name
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "read_index.npy").size == a["config"]["reads_per_gpu"]  # C1's 1 000 reads: all of them
    assert float(np.load(tmp_path / "a" / "read_hit_count.npy").sum()) == np.load(tmp_path / "a" / "hit_lower.npy").size


@pytest.mark.gpu
def test_full_bench_line_keeps_its_reports():
    d = _bench(SMALL + ["--steps", "2", "--full", "--cpu-seconds", "1"])
    assert d["steps"] == 2 and len(d["roofline"]["launch_marks_ms"]) == 2
    assert d["parity"]["bit_identical_hits"] and d["parity"]["identical_event_counters"]
    assert d["cpu_baseline"]["value"] > 0 and d["tail"] is not None and d["e2e"]["identical_to_device_path"]


@pytest.mark.gpu
def test_plain_bench_two_ranks_on_one_gpu_over_gloo():
    """The plain run's N > 1 ending (no gather check, every rank leaves the group): two ranks share device 0."""
    d = _bench(["--gpus", "2", "--dist-backend", "gloo", "--config", "c2", "--genome-bp", "2000000", "--reads", "60000", "--steps", "2", "--warmup", "1",
                "--watchdog-s", "120"])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["value"] > 0 and "gather" not in d
