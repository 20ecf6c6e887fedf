"""Adapter trimming and read-pair merging without a GPU: mapad_merge_pairs_host / mapad_trim_reads_host (mapad_amd/csrc/merge_core.hpp — the source the kernels
compile too) against the rule restated in Python (tests/merge_util.py) on the shared case table; the parameter check; the core driven lane by lane in a
stand-alone program under the address and undefined-behaviour sanitizers (tests/emu/merge_selftest.cpp); and planted truth — what fraction of synthetic pairs the
rule itself gets right, asserted for the Python rule first and then product == Python rule pair by pair."""
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb

import merge_util as mu

_HERE = os.path.dirname(os.path.abspath(__file__))


def c_params(P, mode=0):
    return mb.merge_params(mode=mode, **P)


def host_pairs(P, pairs):
    s1, q1, o1 = mu.pack([(p[0], p[1]) for p in pairs])
    s2, q2, o2 = mu.pack([(p[2], p[3]) for p in pairs])
    return mb.merge_pairs_host(c_params(P), s1, q1, o1, s2, q2, o2)


def host_single(P, reads):
    s, q, o = mu.pack(reads)
    return mb.trim_reads_host(c_params(P, mode=1), s, q, o)


def test_core_selftest_under_sanitizers(tmp_path):
    """64 emulated lanes, ballots into bit planes, shifted words, a candidate per lane — against the serial restatement; in a child process of its own"""
    exe = str(tmp_path / "merge_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(_HERE, "emu", "merge_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "merge selftest ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("group", range(len(mu.case_table())))
def test_pairs_equal_the_rule_on_the_table(group):
    label, P, pairs = mu.case_table()[group]
    want = mu.run_rule(pairs, P)
    got = host_pairs(P, pairs)
    mu.assert_same(got, want, label)
    assert int(got["counts"]["class_counts"].sum()) == len(pairs) == got["counts"]["pairs_seen"]


def test_the_table_reaches_every_class_and_the_limits():
    """what the table is for: every class occurs, fragments past the overlap limit come out unmerged, 512-base mates merge, 513 is too_long, an empty mate is its own"""
    label, P, pairs = mu.case_table()[0]
    got = host_pairs(P, pairs)
    assert all(int(c) > 0 for c in got["counts"]["class_counts"]), got["counts"]["class_counts"]
    lens = [(len(p[0]), len(p[2])) for p in pairs]
    for i, (L1, L2) in enumerate(lens):
        if (L1, L2) == (513, 20):
            assert got["cls"][i] == mu.TOO_LONG
        if (L1, L2) == (0, 30):
            assert got["cls"][i] == mu.EMPTY_MATE
    big = [i for i, l in enumerate(lens) if l == (512, 512)]
    assert any(got["cls"][i] == mu.MERGED and got["frag_len"][i] == 1013 for i in big)  # L1 + L2 - 11
    assert all(got["offsets"][i + 1] == got["offsets"][i] for i in range(len(pairs)) if got["cls"][i] != mu.MERGED)


@pytest.mark.parametrize("group", range(len(mu.single_table())))
def test_single_end_equals_the_rule_on_the_table(group):
    label, P, reads = mu.single_table()[group]
    want = mu.run_rule(reads, P, single=True)
    got = host_single(P, reads)
    mu.assert_same(got, want, label)
    assert int(got["counts"]["class_counts"].sum()) == len(reads)


def test_defaults_are_the_documented_ones():
    p = mb.merge_params()
    assert (p.min_overlap, p.min_adapter_overlap, p.max_mismatch_permille, p.min_length, p.max_quality, p.mode) == (11, 3, 166, 15, 41, 0)
    assert bytes(p.adapter1[:p.adapter1_len]) == mu.A1 and bytes(p.adapter2[:p.adapter2_len]) == mu.A2


@pytest.mark.parametrize("bad", [dict(adapter1=b"A" * 65), dict(adapter2=b"C" * 65), dict(adapter1=b"ACGN"), dict(adapter2=b"ACRT"), dict(adapter1=b"acgt"),
                                 dict(min_overlap=0), dict(min_adapter_overlap=0), dict(max_quality=94), dict(max_mismatch_permille=1001), dict(mode=2)])
def test_params_check_rejects(bad):
    with pytest.raises(mapad_amd.MapadError):
        mb.merge_params(**bad)
    # ... and the entry points refuse such parameters themselves
    p = mb.merge_params()
    for k, v in bad.items():
        if k.startswith("adapter"):
            setattr(p, k + "_len", len(v))
            if len(v) <= mb.MERGE_MAX_ADAPTER:
                mb.C.memmove(getattr(p, k), v, len(v))
        else:
            setattr(p, k, v)
    s, q, o = mu.pack([(b"ACGT" * 10, bytes(40))])
    with pytest.raises(mapad_amd.MapadError):
        mb.merge_pairs_host(p, s, q, o, s, q, o)


def test_params_check_accepts_the_edges():
    mb.merge_params(adapter1=b"A" * 64, adapter2=b"", min_overlap=1, max_quality=93, max_mismatch_permille=1000, min_length=0)
    mb.merge_params(mode=1, adapter1=b"", min_adapter_overlap=1, max_mismatch_permille=0)


def test_a_mode_takes_only_its_own_entry_point():
    s, q, o = mu.pack([(b"ACGT" * 10, bytes(40))])
    with pytest.raises(mapad_amd.MapadError):
        mb.merge_pairs_host(mb.merge_params(mode=1), s, q, o, s, q, o)
    with pytest.raises(mapad_amd.MapadError):
        mb.trim_reads_host(mb.merge_params(mode=0), s, q, o)


def test_no_pairs():
    e = np.zeros(0, np.uint8)
    got = mb.merge_pairs_host(mb.merge_params(), e, e, np.zeros(1, np.uint64), e, e, np.zeros(1, np.uint64))
    assert got["n_pairs"] == 0 and got["offsets"].tolist() == [0] and got["counts"]["pairs_seen"] == 0 and int(got["counts"]["class_counts"].sum()) == 0


# ---- planted truth ----------------------------------------------------------------------------------------------------------------------------------------------
def _planted(seed, L1, L2, n, rate):
    rng = np.random.default_rng(seed)
    pairs, truth = [], []
    for _ in range(n):
        F = int(rng.integers(0, L1 + L2 + 1))
        frag = mu.rand_bases(rng, F)
        r1, q1, r2, q2 = mu.sequence_pair(rng, frag, L1, L2)
        if rate:
            r1, r2 = mu.mutate(rng, r1, rate), mu.mutate(rng, r2, rate)
        pairs.append((r1, q1, r2, q2))
        truth.append(frag)
    return pairs, truth


def _wrong(res, pairs, truth, L1, L2, compare_bases):
    """pairs whose outcome is not the truth: a fragment of at most L1 + L2 - 11 recovered at its length (and, error-free, with its bases), a longer one unmerged"""
    wrong = 0
    for i, frag in enumerate(truth):
        F = len(frag)
        if F > L1 + L2 - 11:
            wrong += res["cls"][i] != mu.UNMERGED
            continue
        ok = res["frag_len"][i] == F and res["cls"][i] == (mu.MERGED if F >= 15 else mu.TOO_SHORT)
        if ok and compare_bases and F >= 15:
            ok = res["seqs"][int(res["offsets"][i]):int(res["offsets"][i + 1])].tobytes() == frag
        wrong += not ok
    return int(wrong)


@pytest.mark.parametrize("L1,L2", [(40, 40), (30, 50)])
def test_planted_fragments_error_free(L1, L2):
    pairs, truth = _planted(100 + L1, L1, L2, 1500, 0.0)
    want = mu.run_rule(pairs)
    assert _wrong(want, pairs, truth, L1, L2, True) == 0  # the rule itself first
    mu.assert_same(host_pairs(mu.DEFAULTS, pairs), want, "error-free")


@pytest.mark.parametrize("L1,L2", [(40, 40), (30, 50)])
def test_planted_fragments_with_one_percent_substitutions(L1, L2):
    pairs, truth = _planted(200 + L1, L1, L2, 1500, 0.01)
    want = mu.run_rule(pairs)
    wrong = _wrong(want, pairs, truth, L1, L2, False)
    print(f"({L1},{L2}): {wrong} of {len(pairs)} pairs differ from the truth")
    assert wrong <= len(pairs) // 100  # at most 1 %: short overlaps pushed past the mismatch share
    mu.assert_same(host_pairs(mu.DEFAULTS, pairs), want, "1 % substitutions")


def test_single_end_planted_adapters():
    """min_adapter_overlap 8: an error-free read with at least 8 adapter bases is cut exactly at the fragment's end; of the adapter-free reads at most 1 % lose
    anything (expected about 5e-4: a chance match of >= 8 columns with at most one mismatch at the read's end)"""
    rng = np.random.default_rng(5)
    P = dict(mu.DEFAULTS, min_adapter_overlap=8)
    L = 60
    with_adapter, free = [], []
    for _ in range(1500):
        F = int(rng.integers(15, L - 8 + 1))
        r1, q1, _, _ = mu.sequence_pair(rng, mu.rand_bases(rng, F), L, 1)
        with_adapter.append((r1, q1, F))
    for _ in range(3000):
        free.append((mu.rand_bases(rng, L), bytes([30]) * L))
    want_a = mu.run_rule([(r, q) for r, q, _ in with_adapter], P, single=True)
    assert all(want_a["cls"][i] == mu.MERGED and want_a["frag_len"][i] == F for i, (_, _, F) in enumerate(with_adapter))
    want_f = mu.run_rule(free, P, single=True)
    trimmed = int((want_f["cls"] != mu.UNMERGED).sum())
    print(f"{trimmed} of {len(free)} adapter-free reads trimmed")
    assert trimmed <= len(free) // 100
    mu.assert_same(host_single(P, [(r, q) for r, q, _ in with_adapter]), want_a, "planted adapters")
    mu.assert_same(host_single(P, free), want_f, "adapter-free")


# ---- the command line, host path ----------------------------------------------------------------------------------------------------------------------------------
def _cli():
    from mapad_amd import build as b
    return b.build_cli()


def _write_fastq(path, names, reads):
    import gzip
    text = "".join(f"@{n} some comment\n{r.decode()}\n+\n{''.join(chr(33 + v) for v in q)}\n" for n, (r, q) in zip(names, reads))
    with (gzip.open(path, "wt") if str(path).endswith(".gz") else open(path, "w")) as f:
        f.write(text)


def _read_fastq(path):
    import gzip
    with (gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)) as f:
        lines = f.read().split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % 4 == 0
    return [(lines[i][1:], lines[i + 1].encode(), bytes(ord(c) - 33 for c in lines[i + 3])) for i in range(0, len(lines) - 1, 4)]


def _cli_pairs(n=300, seed=9):
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n):
        L1, L2 = int(rng.integers(30, 80)), int(rng.integers(30, 80))
        pairs.append(mu.sequence_pair(rng, mu.rand_bases(rng, int(rng.integers(0, 170))), L1, L2))
    return pairs


def _expected_records(want, names, single=False):
    out = []
    for i, name in enumerate(names):
        if want["cls"][i] == mu.MERGED or (single and want["cls"][i] == mu.UNMERGED):
            b, e = int(want["offsets"][i]), int(want["offsets"][i + 1])
            out.append((name, want["seqs"][b:e].tobytes(), want["quals"][b:e].tobytes()))
    return out


def _report(path):
    rows = [ln.split("\t") for ln in open(path).read().splitlines()]
    keys = {k: v for k, v in rows if not k.isdigit()}
    hist = {int(k): int(v) for k, v in rows if k.isdigit()}
    return keys, hist


@pytest.mark.parametrize("ext", ["fastq", "fastq.gz"])
def test_cli_merge_host_writes_what_the_rule_says(tmp_path, ext):
    pairs = _cli_pairs()
    names = [f"read{i}" for i in range(len(pairs))]
    f1, f2, out, rep = (str(tmp_path / x) for x in (f"r1.{ext}", f"r2.{ext}", f"out.{ext}", "report.tsv"))
    _write_fastq(f1, [n + "/1" for n in names], [(p[0], p[1]) for p in pairs])
    _write_fastq(f2, [n + "/2" for n in names], [(p[2], p[3]) for p in pairs])
    # two chunks, and parameters that are not the defaults
    P = dict(mu.DEFAULTS, min_overlap=9, min_length=20, max_quality=50)
    subprocess.run([_cli(), "merge", "-1", f1, "-2", f2, "-o", out, "--host", "--batch_size", "200", "--merge_min_overlap", "9", "--merge_min_length", "20",
                    "--merge_max_quality", "50", "--merge_report", rep], check=True, capture_output=True, timeout=120)
    want = mu.run_rule(pairs, P)
    assert _read_fastq(out) == _expected_records(want, names)
    keys, hist = _report(rep)
    assert int(keys["pairs_seen"]) == len(pairs)
    assert [int(keys[k]) for k in ("merged", "too_short", "unmerged", "empty_mate", "too_long")] == want["counts"]["class_counts"].tolist()
    assert int(keys["bases_in"]) == want["counts"]["bases_in"] and int(keys["bases_out"]) == want["counts"]["bases_out"]
    assert hist == {k: int(v) for k, v in enumerate(want["counts"]["histogram"]) if v}
    merged = int(want["counts"]["class_counts"][0])
    assert abs(float(keys["mean_length"]) - want["counts"]["bases_out"] / merged) < 1e-3


def test_cli_trim_host_single_end(tmp_path):
    rng = np.random.default_rng(3)
    reads = []
    for _ in range(200):
        r1, q1, _, _ = mu.sequence_pair(rng, mu.rand_bases(rng, int(rng.integers(0, 90))), 60, 1)
        reads.append((r1, q1))
    names = [f"s{i}" for i in range(len(reads))]
    f1, out, rep = (str(tmp_path / x) for x in ("r.fastq", "out.fastq", "report.tsv"))
    _write_fastq(f1, names, reads)
    subprocess.run([_cli(), "merge", "-1", f1, "-o", out, "--host", "--trim_min_overlap", "8", "--merge_report", rep], check=True, capture_output=True, timeout=120)
    want = mu.run_rule(reads, dict(mu.DEFAULTS, min_adapter_overlap=8), single=True)
    assert _read_fastq(out) == _expected_records(want, names, single=True)
    keys, _ = _report(rep)
    assert [int(keys[k]) for k in ("trimmed", "too_short", "untouched", "empty_mate", "too_long")] == want["counts"]["class_counts"].tolist()


def test_cli_merge_errors_name_the_record(tmp_path):
    pairs = _cli_pairs(5)
    names = [f"read{i}" for i in range(5)]
    f1, f2, f2short, f2bad, out = (str(tmp_path / x) for x in ("r1.fastq", "r2.fastq", "r2short.fastq", "r2bad.fastq", "out.fastq"))
    _write_fastq(f1, [n + "/1" for n in names], [(p[0], p[1]) for p in pairs])
    _write_fastq(f2short, [n + "/2" for n in names[:3]], [(p[2], p[3]) for p in pairs[:3]])
    bad = [n + "/2" for n in names]
    bad[2] = "other/2"
    _write_fastq(f2bad, bad, [(p[2], p[3]) for p in pairs])
    r = subprocess.run([_cli(), "merge", "-1", f1, "-2", f2short, "-o", out, "--host"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ends at record 4" in r.stderr and "r2short.fastq" in r.stderr, r.stderr
    r = subprocess.run([_cli(), "merge", "-1", f1, "-2", f2bad, "-o", out, "--host"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "names of record 3 differ" in r.stderr and "other/2" in r.stderr, r.stderr
    r = subprocess.run([_cli(), "merge", "-1", f1, "-2", f1, "-o", out, "--host", "--adapter1", "ACGN"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "adapters" in r.stderr, r.stderr


def test_an_invalid_byte_of_mate_2_alone_stays_as_it_is():
    """F > L1: the merged read's positions p >= L1 come from mate 2 alone — comp of a valid base, an invalid byte unchanged, the quality unchanged"""
    rng = np.random.default_rng(8)
    F, L = 100, 70
    frag = mu.rand_bases(rng, F)
    r1, q1, r2, q2 = mu.sequence_pair(rng, frag, L, L)
    r2 = bytearray(r2)
    r2[0], r2[F - L - 1] = ord("R"), ord("N")  # output positions F - 1 and L: the last of the read and the first behind mate 1
    got = host_pairs(mu.DEFAULTS, [(r1, q1, bytes(r2), q2)])
    assert got["cls"][0] == mu.MERGED and got["frag_len"][0] == F
    want = bytearray(frag)
    want[F - 1], want[L] = ord("R"), ord("N")
    assert got["seqs"].tobytes() == bytes(want)
    assert got["quals"][F - 1] == q2[0] and got["quals"][L] == q2[F - L - 1]
    mu.assert_same(got, mu.run_rule([(r1, q1, bytes(r2), q2)]), "mate 2 alone")
