"""bench.py's entry-point contract, as far as it can be checked without a GPU: it refuses to run without a device (no CPU path), a
--gpus N it cannot honour is an error and never a silent 1-GPU run, and a torchrun world that disagrees with --gpus is an error."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=e, timeout=300)


def test_bench_needs_a_gpu_and_prints_nothing_to_stdout_when_it_fails():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("this is the no-GPU contract")
    p = _run(["--steps", "1", "--warmup", "0"])
    assert p.returncode != 0 and "no CPU path" in p.stderr and p.stdout.strip() == ""


def test_bench_gpus_n_without_n_devices_is_an_error():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("needs a box with fewer than two devices")
    p = _run(["--gpus", "2"])
    assert p.returncode == 2 and "--gpus 2" in p.stderr and p.stdout.strip() == ""


def test_bench_world_size_must_match_gpus():
    p = _run(["--gpus", "1"], env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2 and "WORLD_SIZE" in p.stderr


def test_committed_traffic_is_tied_to_the_machine_code_of_the_library():
    """roofline.traffic comes from PMC passes run earlier (profiles/collect.sh); bench.py reports it only while the library's gfx950 machine code is the code
    those passes ran.  The tie is a hash of the device code itself (mapad_amd/build.py: kernel_code_hash) — it must exist for the built library, be the same
    for two reads of it, and every entry that feeds the default line must carry it."""
    import json
    from mapad_amd import build
    build.build()
    h = build.kernel_code_hash()
    assert h and len(h) == 16 and int(h, 16) >= 0 and h == build.kernel_code_hash()
    assert build.kernel_code_hash(os.path.join(ROOT, "no_such_library.so")) is None
    traffic = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    for key in ("c4:3000000000:10000000", "c2:48000000:1000000", "c3:48000000:1000000"):
        assert len(traffic[key].get("kernel_code_sha16", "")) == 16 and traffic[key]["search_kernel"] > 0


def test_bench_has_full_and_dump_outputs_options():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout


def test_threaded_workload_generation_makes_the_same_genome_and_reads():
    """bench.py makes its genome and reads on several host threads: the bytes must be those of the one-thread generators."""
    import numpy as np

    import bench
    from mapad_amd import synth
    n_bp = 2 * (1 << 24) + 12345  # three chunks, the last one partial
    g = synth.genome(n_bp, seed=1234)
    assert np.array_equal(g, synth.genome(n_bp, seed=1234, threads=3))
    kw = dict(qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0))
    one = bench.make_reads(synth, g, 3500, 4325, chunk=1000, **kw)
    many = bench.make_reads(synth, g, 3500, 4325, threads=3, chunk=1000, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(one, many))
    assert int(one[2][-1]) == one[0].size == 3500 * 50


def test_dump_outputs_writes_a_fixed_sample_in_float_within_the_size_limit(tmp_path):
    """--dump-outputs: float32 / float64 .npy files of a seeded sample of the last step's reads, the same sample for the same result, <= 64 MB."""
    import numpy as np

    import bench
    from mapad_amd.binding import COUNTER_DTYPE, HIT_DTYPE

    class Result:  # the fields of mapad_amd.BatchResult that dump_outputs reads
        pass

    rng = np.random.default_rng(7)
    r = Result()
    r.n_reads = 100_000
    counts = rng.integers(0, 4, r.n_reads)
    r.hit_begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    r.n_hits = int(r.hit_begin[-1])
    r.hits_arr = np.zeros(r.n_hits, HIT_DTYPE)
    r.hits_arr["lower"] = rng.integers(0, 6_000_000_000, r.n_hits)
    r.hits_arr["size"] = rng.integers(1, 9, r.n_hits)
    r.hits_arr["score"] = rng.normal(size=r.n_hits).astype(np.float32)
    r.hits_arr["n_ops"] = rng.integers(1, 60, r.n_hits)
    r.hits_arr["ops_offset"] = np.concatenate([[0], np.cumsum(r.hits_arr["n_ops"])[:-1]])
    r.ops = rng.integers(0, 1 << 31, int(r.hits_arr["n_ops"].sum())).astype(np.uint32)
    r.status = rng.integers(0, 32, r.n_reads).astype(np.uint32)
    r.counters = np.zeros(r.n_reads, COUNTER_DTYPE)
    r.counters["n_pop"] = rng.integers(0, 1000, r.n_reads)
    shapes = bench.dump_outputs(r, str(tmp_path / "a"))
    bench.dump_outputs(r, str(tmp_path / "b"))
    total = 0
    for name in shapes:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        total += a.nbytes
    assert total <= bench.DUMP_MAX_BYTES
    idx = np.load(tmp_path / "a" / "read_index.npy").astype(np.int64)
    assert idx.size == bench.DUMP_SAMPLE_READS and np.all(np.diff(idx) > 0)
    hc = np.load(tmp_path / "a" / "read_hit_count.npy")
    assert np.array_equal(hc, counts[idx])
    lower = np.load(tmp_path / "a" / "hit_lower.npy")
    want = np.concatenate([r.hits_arr["lower"][int(r.hit_begin[i]):int(r.hit_begin[i + 1])] for i in idx])
    assert np.array_equal(lower, want.astype(np.float64))
    n_ops = np.load(tmp_path / "a" / "hit_n_ops.npy")
    assert np.load(tmp_path / "a" / "ops.npy").size == int(n_ops.sum())
