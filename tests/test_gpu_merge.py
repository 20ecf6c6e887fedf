"""Adapter trimming and read-pair merging on the GPU (run with -m gpu on an MI355X): merge_decide_kernel / merge_write_kernel and the scan between them against
the host path — the same core on one thread per pair, itself held to the Python rule by tests/test_merge_host.py — byte for byte on the shared case table
(tests/merge_util.py), in both modes; batch sizes around the four wavefronts of a block and the 256 pairs of a scan tile; one set of pairs cut into calls of
different sizes; mapad_merge_pairs_device feeding mapad_map_batch_device on one stream; and a merger living beside a Context."""
import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import presets, synth

import device_util as du
import merge_util as mu

pytestmark = pytest.mark.gpu


def packed_pairs(pairs):
    return mu.pack([(p[0], p[1]) for p in pairs]) + mu.pack([(p[2], p[3]) for p in pairs])


def mixed_pairs(n, seed):
    """mates of 20 .. 120 bases, fragments of 0 .. 260: every class but too_long, 1 % substitutions"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        L1, L2 = int(rng.integers(20, 121)), int(rng.integers(20, 121))
        r1, q1, r2, q2 = mu.sequence_pair(rng, mu.rand_bases(rng, int(rng.integers(0, 261))), L1, L2)
        out.append((mu.mutate(rng, r1, 0.01), q1, mu.mutate(rng, r2, 0.01), q2))
    return out


@pytest.fixture(scope="module")
def thousand():
    pairs = mixed_pairs(1000, 21)
    return pairs, mb.merge_pairs_host(mb.merge_params(), *packed_pairs(pairs))


@pytest.mark.parametrize("group", range(len(mu.case_table())))
def test_pairs_equal_the_host_on_the_table(group):
    label, P, pairs = mu.case_table()[group]
    params = mb.merge_params(**P)
    want = mb.merge_pairs_host(params, *packed_pairs(pairs))
    m = mb.Merger(params)
    try:
        mu.assert_same(m.merge_pairs(*packed_pairs(pairs)), want, label)
    finally:
        m.close()


@pytest.mark.parametrize("group", range(len(mu.single_table())))
def test_single_end_equals_the_host_on_the_table(group):
    label, P, reads = mu.single_table()[group]
    params = mb.merge_params(mode=1, **P)
    want = mb.trim_reads_host(params, *mu.pack(reads))
    m = mb.Merger(params)
    try:
        mu.assert_same(m.trim_reads(*mu.pack(reads)), want, label)
    finally:
        m.close()


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000])
def test_batch_sizes(thousand, n):
    pairs = thousand[0][:n]
    params = mb.merge_params()
    want = mb.merge_pairs_host(params, *packed_pairs(pairs))
    m = mb.Merger(params)
    try:
        got = m.merge_pairs(*packed_pairs(pairs))
        mu.assert_same(got, want, f"{n} pairs")
        assert got["counts"]["pairs_seen"] == n == int(got["counts"]["class_counts"].sum())
    finally:
        m.close()


@pytest.mark.parametrize("cut", [1, 7, 1000])
def test_calls_of_any_size_give_the_same_outputs_and_totals(thousand, cut):
    pairs, want = thousand
    n = len(pairs)
    m = mb.Merger(mb.merge_params())
    try:
        parts = [m.merge_pairs(*packed_pairs(pairs[i:i + cut])) for i in range(0, n, cut)]
        for k in ("cls", "frag_len", "matches", "mismatches", "seqs", "quals"):
            assert np.array_equal(np.concatenate([p[k] for p in parts]), want[k]), k
        assert np.array_equal(np.concatenate([np.diff(p["offsets"].astype(np.int64)) for p in parts]), np.diff(want["offsets"].astype(np.int64)))
        t = m.totals()
        assert t["calls"] == len(parts) and t["pairs_seen"] == n
        for k in ("bases_in", "bases_out"):
            assert t[k] == want["counts"][k], k
        assert np.array_equal(t["class_counts"], want["counts"]["class_counts"]) and np.array_equal(t["histogram"], want["counts"]["histogram"])
        m.reset()
        t = m.totals()
        assert t["calls"] == 0 and t["pairs_seen"] == 0 and int(t["histogram"].sum()) == 0
    finally:
        m.close()


def genome_pairs(genome, n, seed):
    """pairs off fragments of 30 .. 150 bases of the genome, mates of 100: every pair merges (the overlap is at least 50 columns)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        F = int(rng.integers(30, 151))
        at = int(rng.integers(0, len(genome) - F))
        frag = genome[at:at + F].tobytes()
        if rng.random() < 0.5:
            frag = mu.revcomp(frag)
        out.append(mu.sequence_pair(rng, frag, 100, 100, qual=(20, 40)))
    return out


def test_merged_reads_go_to_the_mapper_without_leaving_the_device():
    """mapad_merge_pairs_device, then mapad_map_batch_device on the same stream over the merger's own buffers: hits and tracks equal map_batch of the merged reads
    fetched through the host entry point, and the device offsets equal the host result's"""
    genome = synth.genome(100_000, seed=31)
    pairs = genome_pairs(genome, 256, 32)
    params = mb.merge_params()
    want = mb.merge_pairs_host(params, *packed_pairs(pairs))
    assert (want["cls"] == mu.MERGED).all()
    hip = du.Hip()
    index = mapad_amd.Index.build([("chr1", genome)])
    ctx = mapad_amd.Context(index, mapad_amd.make_params(presets.resolve(presets.DAMAGE)), 0)
    s = hip.stream()
    m = mb.Merger(params)
    try:
        m.set_stream(s)
        ctx.set_stream(s)
        dev = [hip.to_device(a) for a in packed_pairs(pairs)]
        d_seqs, d_quals, d_offs, total = m.merge_pairs_device(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], len(pairs))
        assert total == int(want["offsets"][-1])
        lens = np.diff(want["offsets"].astype(np.int64)).astype(np.uint32)
        ctx.prepare_lengths(lens)
        ctx.map_batch_device(d_seqs, d_quals, d_offs, len(pairs), int(lens.max()))
        got = ctx.fetch()
        hip.synchronize(s)
        assert np.array_equal(hip.from_device(d_offs, len(pairs) + 1, np.uint64), want["offsets"])
        assert np.array_equal(hip.from_device(d_seqs, total, np.uint8), want["seqs"]) and np.array_equal(hip.from_device(d_quals, total, np.uint8), want["quals"])
        ref = ctx.map_batch(want["seqs"], want["quals"], want["offsets"])
        assert np.array_equal(got.hit_begin, ref.hit_begin)
        assert got.hits_arr.tobytes() == ref.hits_arr.tobytes() and np.array_equal(got.ops, ref.ops)
        assert int((np.diff(ref.hit_begin.astype(np.int64)) > 0).sum()) > 200  # the merged reads do map
        t = m.totals()
        assert t["pairs_seen"] == len(pairs) and t["bases_out"] == total
    finally:
        m.close()
        ctx.close()
        hip.release()


def test_a_merger_beside_a_live_context_changes_nothing_of_it(thousand):
    genome = synth.genome(100_000, seed=41)
    seqs, quals, offsets = synth.reads(genome, 128, 50, seed=42, qual_range=(20, 40))
    index = mapad_amd.Index.build([("chr1", genome)])
    ctx = mapad_amd.Context(index, mapad_amd.make_params(presets.resolve(presets.DAMAGE)), 0)
    try:
        before = ctx.map_batch(seqs, quals, offsets)
        m = mb.Merger(mb.merge_params())
        pairs, want = thousand
        mu.assert_same(m.merge_pairs(*packed_pairs(pairs)), want, "beside a context")
        between = ctx.map_batch(seqs, quals, offsets)
        m.reset()
        m.close()
        after = ctx.map_batch(seqs, quals, offsets)
        for r in (between, after):
            assert np.array_equal(r.hit_begin, before.hit_begin) and r.hits_arr.tobytes() == before.hits_arr.tobytes() and np.array_equal(r.ops, before.ops)
    finally:
        ctx.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------------------------
GUARD = ["timeout", "-k", "10", "300"]  # every GPU child process under a time limit of its own
MODEL_FLAGS = ["-l", "single_stranded", "-f", "0.5", "-t", "0.5", "-d", "0.02", "-s", "1.0", "-i", "0.001", "-p", "0.03"]


def _write_fastq(path, names, reads):
    with open(path, "w") as f:
        for n, (r, q) in zip(names, reads):
            f.write(f"@{n}\n{r.decode()}\n+\n{''.join(chr(33 + v) for v in q)}\n")


def _records(path):
    """a BAM's records without what depends on the run: XD is the chunk's wall time per read"""
    from bam_util import read_bam
    recs = read_bam(path)[2]
    for r in recs:
        r["tags"].pop("XD", None)
        r["tag_order"] = [t for t in r["tag_order"] if t != "XD"]
    return recs


def test_cli_map_of_two_files_equals_map_of_the_merged_file(tmp_path):
    """`map -r R1 --reads2 R2` (2 000 pairs, two chunks, damage profile and coverage on) writes the records and the two report files of `map -r merged.fastq`
    over the file `mapad-amd merge` wrote; --merge_report equals the Python rule's counts; --unmerged single adds exactly the /1 and /2 reads"""
    import subprocess

    from mapad_amd import build as mbuild
    mapad_amd.lib()
    cli = mbuild.build_cli()
    genome = synth.genome(100_000, seed=51)
    rng = np.random.default_rng(52)
    pairs = []
    for _ in range(2000):
        F = int(rng.integers(0, 190))  # mates of 80: fragments past 149 do not merge
        at = int(rng.integers(0, len(genome) - 200))
        frag = genome[at:at + F].tobytes()
        r1, q1, r2, q2 = mu.sequence_pair(rng, frag, 80, 80, qual=(20, 40))
        pairs.append((mu.mutate(rng, r1, 0.005), q1, mu.mutate(rng, r2, 0.005), q2))
    names = [f"p{i}" for i in range(len(pairs))]
    fa, f1, f2, merged = (str(tmp_path / x) for x in ("ref.fa", "r1.fastq", "r2.fastq", "merged.fastq"))
    with open(fa, "w") as f:
        f.write(">chr1\n" + "\n".join(genome[i:i + 60].tobytes().decode() for i in range(0, len(genome), 60)) + "\n")
    _write_fastq(f1, [n + "/1" for n in names], [(p[0], p[1]) for p in pairs])
    _write_fastq(f2, [n + "/2" for n in names], [(p[2], p[3]) for p in pairs])
    subprocess.check_call(GUARD + [cli, "index", "-g", fa])

    def out(tag):
        return {k: str(tmp_path / f"{tag}.{k}") for k in ("bam", "damage", "coverage", "report")}
    a, b, c = out("a"), out("b"), out("c")
    stages = lambda o: ["--damage_profile", o["damage"], "--coverage", o["coverage"], "-o", o["bam"], "--batch_size", "1200", "--seed", "7"]  # noqa: E731
    subprocess.check_call(GUARD + [cli, "map", "-r", f1, "--reads2", f2, "-g", fa, "--merge_report", a["report"]] + MODEL_FLAGS + stages(a))
    subprocess.check_call(GUARD + [cli, "merge", "-1", f1, "-2", f2, "-o", merged, "--merge_report", b["report"]])
    subprocess.check_call(GUARD + [cli, "map", "-r", merged, "-g", fa] + MODEL_FLAGS + stages(b))
    want = mu.run_rule(pairs)
    ra, rb = _records(a["bam"]), _records(b["bam"])
    assert len(ra) == int(want["counts"]["class_counts"][0]) > 1000
    assert ra == rb
    assert [r["name"] for r in ra] == [n for i, n in enumerate(names) if want["cls"][i] == mu.MERGED] and all(r["flags"] in (0, 4, 16) for r in ra)
    assert sum(r["flags"] != 4 for r in ra) > 800  # the merged reads map
    for k in ("damage", "coverage", "report"):
        assert open(a[k]).read() == open(b[k]).read(), k
    rows = dict(ln.split("\t") for ln in open(a["report"]).read().splitlines())
    assert int(rows["pairs_seen"]) == len(pairs)
    assert [int(rows[k]) for k in ("merged", "too_short", "unmerged", "empty_mate", "too_long")] == want["counts"]["class_counts"].tolist()
    assert int(rows["bases_in"]) == want["counts"]["bases_in"] and int(rows["bases_out"]) == want["counts"]["bases_out"]
    # --unmerged single: the same records, and between them the mates of the pairs that did not merge, each trimmed by the single-end rule with its own adapter
    subprocess.check_call(GUARD + [cli, "map", "-r", f1, "--reads2", f2, "-g", fa, "--unmerged", "single"] + MODEL_FLAGS + stages(c))
    rc = _records(c["bam"])
    expect = []
    for i, n in enumerate(names):
        if want["cls"][i] == mu.MERGED:
            expect.append(n)
        elif want["cls"][i] >= mu.UNMERGED:
            for tag, mate, qual, adapter in (("/1", pairs[i][0], pairs[i][1], mu.A1), ("/2", pairs[i][2], pairs[i][3], mu.A2)):
                cls, _, _, _, bases, _ = mu.trim_read(mate, qual, dict(mu.DEFAULTS, adapter1=adapter))
                if cls in (mu.MERGED, mu.UNMERGED):
                    expect.append((n + tag, len(bases)))
    assert [r["name"] if "/" not in r["name"] else (r["name"], len(r["seq"])) for r in rc] == expect
    assert [r for r in rc if "/" not in r["name"]] == ra
    assert any("/" in r["name"] for r in rc)


def test_cli_map_trim_adapter_and_refusals(tmp_path):
    import subprocess

    from mapad_amd import build as mbuild
    mapad_amd.lib()
    cli = mbuild.build_cli()
    genome = synth.genome(50_000, seed=61)
    rng = np.random.default_rng(62)
    reads = []
    for _ in range(300):
        F = int(rng.integers(5, 100))
        at = int(rng.integers(0, len(genome) - 200))
        r1, q1, _, _ = mu.sequence_pair(rng, genome[at:at + F].tobytes(), 60, 1, qual=(20, 40))
        reads.append((r1, q1))
    names = [f"s{i}" for i in range(len(reads))]
    fa, fq, bam = (str(tmp_path / x) for x in ("ref.fa", "r.fastq", "out.bam"))
    with open(fa, "w") as f:
        f.write(">chr1\n" + "\n".join(genome[i:i + 60].tobytes().decode() for i in range(0, len(genome), 60)) + "\n")
    _write_fastq(fq, names, reads)
    subprocess.check_call(GUARD + [cli, "index", "-g", fa])
    subprocess.check_call(GUARD + [cli, "map", "-r", fq, "-g", fa, "-o", bam, "--trim_adapter", "--trim_min_overlap", "8"] + MODEL_FLAGS)
    want = mu.run_rule(reads, dict(mu.DEFAULTS, min_adapter_overlap=8), single=True)
    recs = _records(bam)
    keep = [i for i in range(len(reads)) if want["cls"][i] in (mu.MERGED, mu.UNMERGED)]
    assert [(r["name"], len(r["seq"])) for r in recs] == [(names[i], int(want["offsets"][i + 1] - want["offsets"][i])) for i in keep]
    assert 0 < len(keep) < len(reads)
    # a BAM beside --reads2 is refused with a message
    pr = subprocess.run(GUARD + [cli, "map", "-r", bam, "--reads2", fq, "-g", fa, "-o", str(tmp_path / "x.bam")] + MODEL_FLAGS, stderr=subprocess.PIPE, text=True)
    assert pr.returncode != 0 and "FASTQ input only" in pr.stderr
