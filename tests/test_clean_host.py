"""The read clean-up without a GPU: mapad_clean_reads_host (mapad_amd/csrc/clean_core.hpp — the source the kernels compile too) against the rule restated in Python
(tests/clean_util.py) on the shared case table; the parameter check; the counters' sums; the core driven lane by lane in a stand-alone program under the address
and undefined-behaviour sanitizers (tests/emu/clean_selftest.cpp); planted truth — what the rule itself does to random reads, pure repeats and planted tails,
asserted for the Python rule first and then product == Python rule read by read; and the command line's host paths: `clean --host`, `merge --host` with the
clean-up options, the refusals and the report."""
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb

import clean_util as cu
import merge_util as mu

_HERE = os.path.dirname(os.path.abspath(__file__))


def host(ops, P, reads):
    return mb.clean_reads_host(mb.clean_params(ops, **P), *cu.pack(reads))


def test_core_selftest_under_sanitizers(tmp_path):
    """64 emulated lanes through the core's ballot, popcount and shuffle functions against the serial restatement; in a child process of its own"""
    exe = str(tmp_path / "clean_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(_HERE, "emu", "clean_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "clean selftest ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("group", range(len(cu.case_table())))
def test_host_equals_the_rule_on_the_table(group):
    label, ops, P, reads = cu.case_table()[group]
    want = cu.run_rule(reads, ops, P)
    got = host(ops, P, reads)
    cu.assert_same(got, want, label)
    assert got["counts"]["calls"] == 1 and got["kernel_ms"] == (0.0, 0.0)


def test_the_table_reaches_every_class_and_the_limits():
    """what the table is for: under all ops every class occurs; 1024 bases are scored, 1025 are too_long and written whole; an empty read is its own class"""
    label, ops, P, reads = next(g for g in cu.case_table() if g[0] == "all ops")
    got = host(ops, P, reads)
    assert all(int(c) > 0 for c in got["counts"]["class_counts"]), got["counts"]["class_counts"]
    lens = np.diff(got["offsets"].astype(np.int64))
    for i, (r, _) in enumerate(reads):
        if len(r) == 0:
            assert got["cls"][i] == cu.EMPTY
        elif len(r) > 1024:
            assert got["cls"][i] == cu.TOO_LONG and lens[i] == len(r) and got["dust"][i] == 0
        else:
            assert got["cls"][i] < cu.EMPTY
        if got["cls"][i] in (cu.TOO_SHORT, cu.LOW_COMPLEXITY, cu.EMPTY):
            assert lens[i] == 0
        elif got["cls"][i] in (cu.KEPT, cu.TRIMMED):
            assert lens[i] == len(r) - int(got["trim5"][i]) - int(got["trim3"][i]) and (got["cls"][i] == cu.KEPT) == (lens[i] == len(r))
    assert any(len(r) == 1024 and got["cls"][i] == cu.LOW_COMPLEXITY for i, (r, _) in enumerate(reads))  # the repeat deep inside 1024 bases is found


@pytest.mark.parametrize("group", range(len(cu.case_table())))
def test_counters_sum(group):
    """reads_seen = the class sum; and over the reads of the classes that yield a read, run as a batch of their own: bases in minus the three removed figures = bases
    out.  Over all reads the difference is what the dropped reads had left."""
    label, ops, P, reads = cu.case_table()[group]
    got = host(ops, P, reads)
    c = got["counts"]
    assert c["reads_seen"] == len(reads) == int(c["class_counts"].sum())
    assert int(c["length_histogram"].sum()) == int(c["class_counts"][[cu.KEPT, cu.TRIMMED]].sum())  # (a too_long read is past the last bin)
    assert c["bases_poly"] == int(got["poly_len"].sum()) and c["bases_trim5"] == int(got["trim5"].sum())
    assert c["bases_trim3"] == int(got["trim3"].astype(np.int64).sum()) - c["bases_poly"]
    yielding = [reads[i] for i in range(len(reads)) if got["cls"][i] in (cu.KEPT, cu.TRIMMED, cu.TOO_LONG)]
    y = host(ops, P, yielding)["counts"]
    assert y["bases_in"] - y["bases_poly"] - y["bases_trim5"] - y["bases_trim3"] == y["bases_out"]
    assert y["bases_out"] == c["bases_out"] and int(y["class_counts"][[cu.TOO_SHORT, cu.LOW_COMPLEXITY, cu.EMPTY]].sum()) == 0
    left = sum(len(r) - int(got["trim5"][i]) - int(got["trim3"][i]) for i, (r, _) in enumerate(reads) if got["cls"][i] in (cu.TOO_SHORT, cu.LOW_COMPLEXITY))
    assert c["bases_in"] - c["bases_poly"] - c["bases_trim5"] - c["bases_trim3"] == c["bases_out"] + left


def test_defaults_are_the_documented_ones():
    p = mb.clean_params()
    assert (p.ops, p.poly_base, p.poly_min_len, p.poly_one_in, p.poly_max_mismatch, p.min_quality, p.min_length, p.max_dust) == (0, ord("G"), 10, 8, 5, 2, 15, 1000)
    assert mb.clean_params(["poly", "dust"]).ops == 9


@pytest.mark.parametrize("bad", [dict(poly_base=ord("N")), dict(poly_base=ord("g")), dict(poly_base=0), dict(poly_base=ord("G") + 256), dict(poly_min_len=0), dict(poly_one_in=0),
                                 dict(min_quality=94), dict(max_dust=1001), dict(ops=16), dict(ops=0x80000001)])
def test_params_check_rejects(bad):
    with pytest.raises(mapad_amd.MapadError):
        mb.clean_params(**bad)
    # ... and the entry point refuses such parameters itself
    p = mb.clean_params(cu.ALL)
    for k, v in bad.items():
        setattr(p, k, v)
    s, q, o = cu.pack([(b"ACGT" * 10, bytes(40))])
    with pytest.raises(mapad_amd.MapadError):
        mb.clean_reads_host(p, s, q, o)


def test_params_check_accepts_the_edges():
    for base in b"ACGT":
        mb.clean_params(cu.ALL, poly_base=base)
    mb.clean_params(15, poly_min_len=1, poly_one_in=1, poly_max_mismatch=0, min_quality=93, max_dust=1000, min_length=0)
    mb.clean_params(0, poly_min_len=2 ** 32 - 1, poly_one_in=2 ** 32 - 1, poly_max_mismatch=2 ** 32 - 1, min_quality=0, max_dust=0, min_length=2 ** 32 - 1)


def test_no_reads():
    e = np.zeros(0, np.uint8)
    got = mb.clean_reads_host(mb.clean_params(cu.ALL), e, e, np.zeros(1, np.uint64))
    assert got["n_reads"] == 0 and got["offsets"].tolist() == [0] and got["counts"]["reads_seen"] == 0 and int(got["counts"]["class_counts"].sum()) == 0


def test_the_scores_of_pure_repeats():
    """a full window of 62 triplets: a homopolymer has one triplet 62 times — 1000; period 2 has two triplets 31 times each — 491; period 3 three triplets 21, 21
    and 20 times — 322; period 4 four triplets 16, 16, 15 and 15 times — 237"""
    for unit, score in ((b"A", 1000), (b"AC", 2000 * 2 * 465 // 3782), (b"ACG", 2000 * (210 + 210 + 190) // 3782), (b"ACGT", 2000 * (120 + 120 + 105 + 105) // 3782)):
        r = (unit * 64)[:64]
        assert cu.dust_score(r) == score
        assert host(cu.DUST, cu.DEFAULTS, [(r, cu.q30(64))])["dust"][0] == score
    assert [cu.dust_score((u * 64)[:64]) for u in (b"A", b"AC", b"ACG", b"ACGT")] == [1000, 491, 322, 237]


# ---- planted truth ----------------------------------------------------------------------------------------------------------------------------------------------
def test_random_reads_are_left_alone():
    """4 000 uniform random reads of 30 to 150 bases, max_dust 70 and the poly-G step: at most 0.5 % dropped, at most 0.5 % poly-trimmed (a random tail needs nine G
    in its last ten bases, about 3e-5; a random window's score has a mean of about 20)"""
    rng = np.random.default_rng(71)
    reads = [(cu.rand_bases(rng, int(rng.integers(30, 151))), cu.q30(1)) for _ in range(4000)]
    reads = [(r, cu.q30(len(r))) for r, _ in reads]
    ops = cu.POLY | cu.DUST
    want = cu.run_rule(reads, ops)
    dropped = int((want["cls"] >= cu.TOO_SHORT).sum())
    poly = int((want["poly_len"] > 0).sum())
    print(f"{dropped} of {len(reads)} random reads dropped, {poly} poly-trimmed, mean dust {want['dust'].mean():.1f}, max {want['dust'].max()}")
    assert dropped <= len(reads) // 200 and poly <= len(reads) // 200
    cu.assert_same(host(ops, cu.DEFAULTS, reads), want, "random reads")


def test_pure_repeats_are_dropped():
    rng = np.random.default_rng(72)
    reads = []
    for period in (1, 2, 3, 4):
        for _ in range(100):
            unit = cu.rand_bases(rng, period)
            L = int(rng.integers(30, 151))
            reads.append(((unit * L)[:L], cu.q30(L)))
    want = cu.run_rule(reads, cu.DUST)
    assert (want["cls"] == cu.LOW_COMPLEXITY).all(), np.flatnonzero(want["cls"] != cu.LOW_COMPLEXITY)[:8]
    cu.assert_same(host(cu.DUST, cu.DEFAULTS, reads), want, "pure repeats")


def test_planted_tails_are_cut_at_the_planted_point():
    """a G tail of 10 or more bases without a mismatch: cut exactly there.  The rule lets a tail run on across up to poly_max_mismatch = 5 other bases (at most one in
    eight), so a G among the first six bases in front of the tail would belong to it by the rule itself: the planted tails stand behind six bases that are not G"""
    rng = np.random.default_rng(73)
    reads, tails = [], []
    for _ in range(1000):
        t = int(rng.integers(10, 140))
        body = cu.rand_bases(rng, int(rng.integers(0, 120))) + bytes(rng.choice(np.frombuffer(b"ACT", np.uint8), 6).tobytes())
        reads.append((body + b"G" * t, cu.q30(len(body) + t)))
        tails.append(t)
    want = cu.run_rule(reads, cu.POLY, dict(cu.DEFAULTS, min_length=0))
    assert want["poly_len"].tolist() == tails and want["trim3"].tolist() == tails and (want["cls"] == cu.TRIMMED).all()
    cu.assert_same(host(cu.POLY, dict(cu.DEFAULTS, min_length=0), reads), want, "planted tails")


def test_mixed_reads_equal_the_rule():
    reads = cu.mixed_reads(1500, 74)
    want = cu.run_rule(reads, cu.ALL)
    assert all(int(c) > 20 for c in want["counts"]["class_counts"][:4])
    cu.assert_same(host(cu.ALL, cu.DEFAULTS, reads), want, "mixed reads")


# ---- the command line, host path ----------------------------------------------------------------------------------------------------------------------------------
def _cli():
    from mapad_amd import build as b
    return b.build_cli()


@pytest.mark.parametrize("ext", ["fastq", "fastq.gz"])
def test_cli_clean_host_writes_what_the_rule_says(tmp_path, ext):
    reads = cu.cli_reads(500, 75)
    names = [f"read{i}" for i in range(len(reads))]
    fq, out, rep = (str(tmp_path / x) for x in (f"r.{ext}", f"out.{ext}", "report.tsv"))
    cu.write_fastq(fq, names, reads)
    # two chunks, and parameters that are not the defaults
    P = dict(cu.DEFAULTS, poly_min_len=8, min_quality=5, min_length=20, max_dust=100)
    subprocess.run([_cli(), "clean", "-1", fq, "-o", out, "--host", "--batch_size", "300", "--trim_poly_g", "--poly_min_length", "8", "--trim_ns", "--trim_qualities",
                    "--min_quality", "5", "--max_dust", "100", "--clean_min_length", "20", "--clean_report", rep], check=True, capture_output=True, timeout=120)
    want = cu.run_rule(reads, cu.ALL, P)
    assert cu.read_fastq(out) == cu.expected_records(want, names)
    assert 0 < len(cu.expected_records(want, names)) < len(reads)
    keys = cu.check_report(rep, want)
    assert "mates_seen" not in keys


@pytest.mark.parametrize("flags,ops", [(["--trim_poly_g"], cu.POLY), (["--trim_ns"], cu.TRIM_N), (["--trim_qualities"], cu.TRIM_QUAL), (["--max_dust", "70"], cu.DUST)])
def test_cli_clean_host_every_op_alone(tmp_path, flags, ops):
    reads = cu.cli_reads(200, 76)
    names = [f"read{i}" for i in range(len(reads))]
    fq, out = str(tmp_path / "r.fastq"), str(tmp_path / "out.fastq")
    cu.write_fastq(fq, names, reads)
    subprocess.run([_cli(), "clean", "-1", fq, "-o", out, "--host"] + flags, check=True, capture_output=True, timeout=120)
    assert cu.read_fastq(out) == cu.expected_records(cu.run_rule(reads, ops), names)


def test_cli_merge_host_with_the_clean_options(tmp_path):
    pairs = cu.tailed_pairs(400, 77)
    names = [f"p{i}" for i in range(len(pairs))]
    f1, f2, out, rep, plain = (str(tmp_path / x) for x in ("r1.fastq", "r2.fastq", "out.fastq", "report.tsv", "plain.fastq"))
    cu.write_fastq(f1, [n + "/1" for n in names], [(p[0], p[1]) for p in pairs])
    cu.write_fastq(f2, [n + "/2" for n in names], [(p[2], p[3]) for p in pairs])
    subprocess.run([_cli(), "merge", "-1", f1, "-2", f2, "-o", out, "--host", "--batch_size", "150", "--trim_poly_g", "--trim_ns", "--trim_qualities", "--max_dust", "70",
                    "--clean_report", rep], check=True, capture_output=True, timeout=120)
    want, front, back = cu.expected_merge_with_clean(pairs, names, cu.ALL)
    got = cu.read_fastq(out)
    assert got == want
    keys = cu.check_report(rep, back)
    assert (keys["mates_seen"], keys["mates_trimmed"], keys["mates_bases_in"], keys["mates_bases_poly"]) == (2 * len(pairs), front["trimmed"], front["bases_in"], front["bases_poly"])
    assert front["trimmed"] > 100 and int(back["counts"]["class_counts"][cu.LOW_COMPLEXITY]) > 10 and int(back["counts"]["class_counts"][cu.TRIMMED]) > 10
    # the poly-G step is what lets the tailed pairs merge: without it fewer reads come out
    subprocess.run([_cli(), "merge", "-1", f1, "-2", f2, "-o", plain, "--host"], check=True, capture_output=True, timeout=120)
    assert len(cu.read_fastq(plain)) < len(got) + int(back["counts"]["class_counts"][[cu.TOO_SHORT, cu.LOW_COMPLEXITY]].sum())
    # poly-G alone beside a merger: one pass, over the mates; its counters are the report's
    subprocess.run([_cli(), "merge", "-1", f1, "-2", f2, "-o", out, "--host", "--trim_poly_g", "--clean_report", rep], check=True, capture_output=True, timeout=120)
    want, front, _ = cu.expected_merge_with_clean(pairs, names, cu.POLY)
    assert cu.read_fastq(out) == want
    keys, _, dust = cu.read_report(rep)
    assert keys["reads_seen"] == 2 * len(pairs) and keys["trimmed"] == front["trimmed"] and keys["bases_poly"] == front["bases_poly"] and dust == {} and "mates_seen" not in keys


def test_cli_refusals(tmp_path):
    reads = cu.cli_reads(5, 78)
    fq, out = str(tmp_path / "r.fastq"), str(tmp_path / "out.fastq")
    cu.write_fastq(fq, [f"r{i}" for i in range(5)], reads)

    def refused(args, word):
        r = subprocess.run([_cli()] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)
    clean = ["clean", "-1", fq, "-o", out, "--host"]
    refused(clean, "nothing to do")
    refused(clean + ["--min_quality", "5", "--trim_ns"], "--min_quality does nothing without --trim_qualities")
    refused(clean + ["--poly_min_length", "12", "--trim_ns"], "--poly_min_length does nothing without --trim_poly_g")
    refused(clean + ["--clean_min_length", "20"], "--clean_min_length does nothing")
    refused(clean + ["--clean_report", str(tmp_path / "x.tsv")], "--clean_report does nothing")
    refused(clean + ["--max_dust", "1001"], "--max_dust <= 1000")
    refused(clean + ["--max_dust", "seventy"], "takes a number")
    refused(clean + ["--trim_qualities", "--min_quality", "94"], "--min_quality <= 93")
    refused(clean + ["--trim_poly_g", "--poly_min_length", "0"], "--poly_min_length >= 1")
    refused(clean + ["--trim_ns", "-2", fq], "one file at a time")
    merge = ["merge", "-1", fq, "-2", fq, "-o", out, "--host"]
    refused(merge + ["--min_quality", "5"], "--min_quality does nothing without --trim_qualities")
    refused(merge + ["--clean_min_length", "20"], "--clean_min_length does nothing")
    # BAM input: the magic bytes of a BGZF block are enough for the reader to take the file for one
    bam = str(tmp_path / "r.bam")
    import gzip
    with gzip.open(bam, "wb") as f:
        f.write(b"BAM\x01" + bytes(8))
    refused(["clean", "-1", bam, "-o", out, "--host", "--trim_ns"], "FASTQ input only")
