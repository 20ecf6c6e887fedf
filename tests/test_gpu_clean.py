"""The read clean-up on the GPU (run with -m gpu on an MI355X): clean_decide_kernel / clean_write_kernel and the scan between them against the host path — the same
core on one thread per read, itself held to the Python rule by tests/test_clean_host.py — byte for byte on the shared case table (tests/clean_util.py); batch
sizes around the four wavefronts of a block and the 256 reads of a scan tile; one set of reads cut into calls of different sizes; mapad_clean_reads_device feeding
mapad_map_batch_device and fed by mapad_merge_pairs_device on one stream; a cleaner living beside a Context and a Merger; and the command line."""
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import presets, synth

import clean_util as cu
import device_util as du
import merge_util as mu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def thousand():
    reads = cu.mixed_reads(1000, 81)
    return reads, mb.clean_reads_host(mb.clean_params(cu.ALL, **cu.DEFAULTS), *cu.pack(reads))


def same_counts(got, want, what):
    for k in cu.COUNTERS:
        assert int(got[k]) == int(want[k]), f"{what}: {k}"
    for k in ("class_counts", "length_histogram", "dust_histogram"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k}"


@pytest.mark.parametrize("group", range(len(cu.case_table())))
def test_device_equals_the_host_on_the_table(group):
    label, ops, P, reads = cu.case_table()[group]
    params = mb.clean_params(ops, **P)
    want = mb.clean_reads_host(params, *cu.pack(reads))
    c = mb.Cleaner(params)
    try:
        got = c.clean_reads(*cu.pack(reads))
        cu.assert_same(got, want, label)
        assert got["kernel_ms"][0] > 0 and got["kernel_ms"][1] > 0
    finally:
        c.close()


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000])
def test_batch_sizes(thousand, n):
    reads = thousand[0][:n]
    params = mb.clean_params(cu.ALL, **cu.DEFAULTS)
    want = mb.clean_reads_host(params, *cu.pack(reads))
    c = mb.Cleaner(params)
    try:
        got = c.clean_reads(*cu.pack(reads))
        cu.assert_same(got, want, f"{n} reads")
        assert got["counts"]["reads_seen"] == n == int(got["counts"]["class_counts"].sum())
    finally:
        c.close()


@pytest.mark.parametrize("cut", [1, 7, 1000])
def test_calls_of_any_size_give_the_same_outputs_and_totals(thousand, cut):
    reads, want = thousand
    n = len(reads)
    c = mb.Cleaner(mb.clean_params(cu.ALL, **cu.DEFAULTS))
    try:
        parts = [c.clean_reads(*cu.pack(reads[i:i + cut])) for i in range(0, n, cut)]
        for k in ("cls", "trim5", "trim3", "poly_len", "dust", "seqs", "quals"):
            assert np.array_equal(np.concatenate([p[k] for p in parts]), want[k]), k
        assert np.array_equal(np.concatenate([np.diff(p["offsets"].astype(np.int64)) for p in parts]), np.diff(want["offsets"].astype(np.int64)))
        t = c.totals()
        assert t["calls"] == len(parts)
        same_counts(t, want["counts"], f"calls of {cut}")
        c.reset()
        t = c.totals()
        assert t["calls"] == 0 and t["reads_seen"] == 0 and int(t["length_histogram"].sum()) == 0 and int(t["dust_histogram"].sum()) == 0
    finally:
        c.close()


def surviving_reads(genome, n, seed):
    """reads of 40 .. 100 bases off the genome with a poly-G tail, an N in front and low qualities behind: every one is trimmed and none is dropped"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.integers(40, 101))
        while True:  # a stretch whose last six bases are not G: the tail behind it is cut where it was planted, and the read left is the genome's
            at = int(rng.integers(0, len(genome) - L))
            core = genome[at:at + L].tobytes()
            if b"G" not in core[-6:]:
                break
        r = b"N" * (i % 3) + core + b"G" * (12 + i % 30)
        q = bytearray(rng.integers(20, 41, len(r), dtype=np.uint8).tobytes())
        q[:i % 3] = bytes(i % 3)
        out.append((r, bytes(q)))
    return out


def test_cleaned_reads_go_to_the_mapper_without_leaving_the_device():
    """mapad_clean_reads_device, then mapad_map_batch_device on the same stream over the cleaner's own buffers: hits and operations equal map_batch of the cleaned
    reads fetched through the host entry point, and the device outputs equal the host result's"""
    genome = synth.genome(100_000, seed=83)
    reads = surviving_reads(genome, 256, 84)
    params = mb.clean_params(cu.ALL, **cu.DEFAULTS)
    want = mb.clean_reads_host(params, *cu.pack(reads))
    assert (want["cls"] == cu.TRIMMED).all() and (want["poly_len"] >= 12).all()
    hip = du.Hip()
    index = mapad_amd.Index.build([("chr1", genome)])
    ctx = mapad_amd.Context(index, mapad_amd.make_params(presets.resolve(presets.DAMAGE)), 0)
    s = hip.stream()
    c = mb.Cleaner(params)
    try:
        c.set_stream(s)
        ctx.set_stream(s)
        dev = [hip.to_device(a) for a in cu.pack(reads)]
        d_seqs, d_quals, d_offs, total = c.clean_reads_device(dev[0], dev[1], dev[2], len(reads))
        assert total == int(want["offsets"][-1])
        lens = np.diff(want["offsets"].astype(np.int64)).astype(np.uint32)
        ctx.prepare_lengths(lens)
        ctx.map_batch_device(d_seqs, d_quals, d_offs, len(reads), int(lens.max()))
        got = ctx.fetch()
        hip.synchronize(s)
        assert np.array_equal(hip.from_device(d_offs, len(reads) + 1, np.uint64), want["offsets"])
        assert np.array_equal(hip.from_device(d_seqs, total, np.uint8), want["seqs"]) and np.array_equal(hip.from_device(d_quals, total, np.uint8), want["quals"])
        ref = ctx.map_batch(want["seqs"], want["quals"], want["offsets"])
        assert np.array_equal(got.hit_begin, ref.hit_begin)
        assert got.hits_arr.tobytes() == ref.hits_arr.tobytes() and np.array_equal(got.ops, ref.ops)
        assert int((np.diff(ref.hit_begin.astype(np.int64)) > 0).sum()) > 200  # the cleaned reads do map
        t = c.totals()
        assert t["reads_seen"] == len(reads) and t["bases_out"] == total
        same_counts(t, want["counts"], "device-resident call")
    finally:
        c.close()
        ctx.close()
        hip.release()


def test_merged_reads_go_to_the_cleaner_on_the_mergers_stream():
    """mapad_merge_pairs_device into mapad_clean_reads_device on the merger's stream: the cleaner reads the merger's own buffers, zero-length slots of unmerged
    pairs included (they come out as empty)"""
    pairs = cu.tailed_pairs(300, 85)
    mparams, cparams = mb.merge_params(), mb.clean_params(cu.TRIM_N | cu.TRIM_QUAL | cu.DUST, **cu.DEFAULTS)
    merged = mb.merge_pairs_host(mparams, *(mu.pack([(p[0], p[1]) for p in pairs]) + mu.pack([(p[2], p[3]) for p in pairs])))
    want = mb.clean_reads_host(cparams, merged["seqs"], merged["quals"], merged["offsets"])
    assert int(want["counts"]["class_counts"][cu.EMPTY]) > 0 and int(want["counts"]["class_counts"][[cu.KEPT, cu.TRIMMED]].sum()) > 100
    hip = du.Hip()
    s = hip.stream()
    m, c = mb.Merger(mparams), mb.Cleaner(cparams)
    try:
        m.set_stream(s)
        c.set_stream(s)
        dev = [hip.to_device(a) for a in mu.pack([(p[0], p[1]) for p in pairs]) + mu.pack([(p[2], p[3]) for p in pairs])]
        ms, mq, mo, _ = m.merge_pairs_device(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], len(pairs))
        d_seqs, d_quals, d_offs, total = c.clean_reads_device(ms, mq, mo, len(pairs))
        hip.synchronize(s)
        assert total == int(want["offsets"][-1])
        assert np.array_equal(hip.from_device(d_offs, len(pairs) + 1, np.uint64), want["offsets"])
        assert np.array_equal(hip.from_device(d_seqs, total, np.uint8), want["seqs"]) and np.array_equal(hip.from_device(d_quals, total, np.uint8), want["quals"])
        same_counts(c.totals(), want["counts"], "behind the merger")
    finally:
        c.close()
        m.close()
        hip.release()


def test_a_cleaner_beside_a_live_context_and_a_merger_changes_nothing_of_them(thousand):
    genome = synth.genome(100_000, seed=86)
    seqs, quals, offsets = synth.reads(genome, 128, 50, seed=87, qual_range=(20, 40))
    pairs = cu.tailed_pairs(100, 88)
    packed = mu.pack([(p[0], p[1]) for p in pairs]) + mu.pack([(p[2], p[3]) for p in pairs])
    index = mapad_amd.Index.build([("chr1", genome)])
    ctx = mapad_amd.Context(index, mapad_amd.make_params(presets.resolve(presets.DAMAGE)), 0)
    m = mb.Merger(mb.merge_params())
    try:
        before = ctx.map_batch(seqs, quals, offsets)
        merged_before = m.merge_pairs(*packed)
        c = mb.Cleaner(mb.clean_params(cu.ALL, **cu.DEFAULTS))
        reads, want = thousand
        cu.assert_same(c.clean_reads(*cu.pack(reads)), want, "beside a context and a merger")
        between = ctx.map_batch(seqs, quals, offsets)
        mu.assert_same(m.merge_pairs(*packed), merged_before, "the merger beside a cleaner")
        cu.assert_same(c.clean_reads(*cu.pack(reads)), want, "a second call")
        c.reset()
        c.close()
        after = ctx.map_batch(seqs, quals, offsets)
        for r in (between, after):
            assert np.array_equal(r.hit_begin, before.hit_begin) and r.hits_arr.tobytes() == before.hits_arr.tobytes() and np.array_equal(r.ops, before.ops)
    finally:
        m.close()
        ctx.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------------------------
GUARD = ["timeout", "-k", "10", "300"]  # every GPU child process under a time limit of its own
MODEL_FLAGS = ["-l", "single_stranded", "-f", "0.5", "-t", "0.5", "-d", "0.02", "-s", "1.0", "-i", "0.001", "-p", "0.03"]
CLEAN_FLAGS = ["--trim_poly_g", "--trim_ns", "--trim_qualities", "--max_dust", "70"]


def _cli():
    from mapad_amd import build as mbuild
    mapad_amd.lib()
    return mbuild.build_cli()


def _records(path):
    """a BAM's records without what depends on the run: XD is the chunk's wall time per read"""
    from bam_util import read_bam
    recs = read_bam(path)[2]
    for r in recs:
        r["tags"].pop("XD", None)
        r["tag_order"] = [t for t in r["tag_order"] if t != "XD"]
    return recs


def _fasta(path, genome):
    with open(path, "w") as f:
        f.write(">chr1\n" + "\n".join(genome[i:i + 60].tobytes().decode() for i in range(0, len(genome), 60)) + "\n")


def test_cli_clean_equals_clean_host(tmp_path):
    reads = cu.cli_reads(1500, 89)
    names = [f"read{i}" for i in range(len(reads))]
    fq, dev, host, rep_d, rep_h = (str(tmp_path / x) for x in ("r.fastq", "dev.fastq", "host.fastq", "dev.tsv", "host.tsv"))
    cu.write_fastq(fq, names, reads)
    flags = CLEAN_FLAGS + ["--batch_size", "600"]
    subprocess.check_call(GUARD + [_cli(), "clean", "-1", fq, "-o", dev, "--clean_report", rep_d] + flags)
    subprocess.check_call([_cli(), "clean", "-1", fq, "-o", host, "--host", "--clean_report", rep_h] + flags)
    assert open(dev).read() == open(host).read() and open(rep_d).read() == open(rep_h).read()
    want = cu.run_rule(reads, cu.ALL)
    cu.check_report(rep_d, want)
    assert 0 < len(cu.read_fastq(dev)) < len(reads)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """a genome with its index files, 1 200 pairs off it as two FASTQ files, and the file `merge --host` writes from them with the four clean-up options"""
    d = tmp_path_factory.mktemp("clean_cli")
    cli = _cli()
    genome = synth.genome(100_000, seed=91)
    pairs = cu.tailed_pairs(1200, 92, genome)
    names = [f"p{i}" for i in range(len(pairs))]
    fa, f1, f2, merged, report = (str(d / x) for x in ("ref.fa", "r1.fastq", "r2.fastq", "merged.fastq", "merged.tsv"))
    _fasta(fa, genome)
    cu.write_fastq(f1, [n + "/1" for n in names], [(p[0], p[1]) for p in pairs])
    cu.write_fastq(f2, [n + "/2" for n in names], [(p[2], p[3]) for p in pairs])
    subprocess.check_call(GUARD + [cli, "index", "-g", fa])
    subprocess.check_call([cli, "merge", "-1", f1, "-2", f2, "-o", merged, "--host", "--clean_report", report] + CLEAN_FLAGS)
    return dict(cli=cli, dir=d, fa=fa, f1=f1, f2=f2, merged=merged, report=report, pairs=pairs, names=names, tail=MODEL_FLAGS + ["--batch_size", "700", "--seed", "7"])


def test_cli_map_of_two_files_with_clean_up_equals_map_of_the_cleaned_file(world):
    """`map -r R1 --reads2 R2` with the four clean-up options (1 200 pairs, two chunks) writes the records of `map -r merged.fastq` over the file `merge --host` wrote
    with the same options, and the same report; the merged file is what the rules in Python say"""
    w = world
    a, b, rep_a = (str(w["dir"] / x) for x in ("a.bam", "b.bam", "a.tsv"))
    subprocess.check_call(GUARD + [w["cli"], "map", "-r", w["f1"], "--reads2", w["f2"], "-g", w["fa"], "-o", a, "--clean_report", rep_a] + CLEAN_FLAGS + w["tail"])
    subprocess.check_call(GUARD + [w["cli"], "map", "-r", w["merged"], "-g", w["fa"], "-o", b] + w["tail"])
    want, front, back = cu.expected_merge_with_clean(w["pairs"], w["names"], cu.ALL)
    assert cu.read_fastq(w["merged"]) == want
    ra, rb = _records(a), _records(b)
    assert ra == rb
    assert [(r["name"], len(r["seq"])) for r in ra] == [(n, len(s)) for n, s, _ in want] and len(ra) > 600
    assert sum(r["flags"] != 4 for r in ra) > 400  # the cleaned reads map
    assert open(rep_a).read() == open(w["report"]).read()
    check = cu.check_report(rep_a, back)
    assert check["mates_seen"] == 2 * len(w["pairs"]) and check["mates_bases_poly"] == front["bases_poly"]


def test_cli_map_with_the_filter_alone_and_refusals(world):
    """without a merge stage: `map -r FILE --max_dust 40 --clean_min_length 40` writes the records of `map` over the file `clean --host` wrote with the same options;
    a BAM beside a clean-up option is refused with a message"""
    w = world
    c, d, cleaned = (str(w["dir"] / x) for x in ("c.bam", "d.bam", "cleaned.fastq"))
    opts = ["--max_dust", "40", "--clean_min_length", "40"]
    subprocess.check_call(GUARD + [w["cli"], "map", "-r", w["merged"], "-g", w["fa"], "-o", c] + opts + w["tail"])
    subprocess.check_call([w["cli"], "clean", "-1", w["merged"], "-o", cleaned, "--host"] + opts)
    subprocess.check_call(GUARD + [w["cli"], "map", "-r", cleaned, "-g", w["fa"], "-o", d] + w["tail"])
    rc, rd = _records(c), _records(d)
    n_in, n_out = len(cu.read_fastq(w["merged"])), len(cu.read_fastq(cleaned))
    assert rc == rd and len(rc) == n_out and 0 < n_out < n_in
    pr = subprocess.run(GUARD + [w["cli"], "map", "-r", c, "-g", w["fa"], "-o", str(w["dir"] / "x.bam"), "--trim_ns"] + MODEL_FLAGS, stderr=subprocess.PIPE, text=True)
    assert pr.returncode != 0 and "FASTQ input only" in pr.stderr
