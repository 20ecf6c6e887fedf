"""The mappability stage on the host (mapad_mappability_host, mapad_mappability_summary_host, `mapad-amd mappability --host`) against the rule in plain Python."""
import os
import subprocess

import numpy as np
import pytest

import mapad_amd
import mappability_util as U


def _seqs(name):
    return [s.encode() for _, s in U.CASES[name][0]]


def test_core_selftest_under_sanitizers(tmp_path):
    """staging, count_start with the scalar rank queries, the palindrome rule and the cover's bit ranges against brute force, in a child process of its own"""
    exe = str(tmp_path / "mappability_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-pthread", "-o", exe, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "mappability_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mappability selftest ok" in out.stdout, out.stdout + out.stderr


def test_the_text_from_the_bwt_is_the_reference_where_it_is_unambiguous():
    for name, (contigs, _) in U.CASES.items():
        ref = "".join(s for _, s in contigs).upper()
        halves = U.case_text(name)
        fwd = [h for h in halves if all(a == b for a, b in zip(h, ref) if b in "ACGT")]
        assert fwd and len(fwd[0]) == len(ref), name
    amb = [h for h in U.case_text("ambiguous") if "X" * 25 in h]
    assert len(amb) == 2 and all("X" * 26 not in h for h in amb)  # the long run is X, the short one was drawn


@pytest.mark.parametrize("name,k,e", U.PARAMS)
def test_host_equals_the_rule(name, k, e):
    index, exp = U.case_index(name), U.expected(name, k, e)
    for tid, seq in enumerate(_seqs(name)):
        counts, cover = mapad_amd.mappability_host(index, tid, seq, k=k, e=e)
        assert counts.tobytes() == exp[tid][0].tobytes(), (tid, "counts")
        assert cover.tobytes() == exp[tid][1].tobytes(), (tid, "cover")
        vc, vv = mapad_amd.mappability_host(index, tid, seq, k=k, e=e, verify=True)  # the right sequence passes and changes nothing
        assert vc.tobytes() == counts.tobytes() and vv.tobytes() == cover.tobytes()
        valid = np.array([p + k <= len(seq) and all(ch in b"ACGTacgt" for ch in seq[p:p + k]) for p in range(len(seq))], bool).reshape(-1)
        assert np.array_equal(counts >= 1, valid)
    got = mapad_amd.mappability_summary_host(index, _seqs(name), k=k, e=e)
    want = U.expected_figures(name, k, e)
    assert [{key: c[key] for key in want[0]} for c in got["contigs"]] == want
    assert got["total"] == U.add_figures(want) and (got["k"], got["e"]) == (k, e)
    assert [c["name"] for c in got["contigs"]] == [n for n, _ in U.CASES[name][0]]


def test_the_table_reaches_what_it_is_there_for():
    c = U.expected("saturation", 4, 0)[0][0]
    assert c.max() == 255 and c[0] == 255 and c[500] == 255   # AAAA and TTTT: both strands add up beyond a byte
    c = U.expected("planted", 35, 0)[0][0]
    assert (c == 2).sum() >= 10 and (c == 1).sum() >= 100     # the exact and the reverse-complement repeat
    assert (U.expected("planted", 35, 1)[0][0] >= 3).sum() >= 1  # ... and the copy with one substitution
    seq = U.CASES["palindrome_once"][0][0][1]
    p = seq.index("GAATTC")
    assert U.expected("palindrome_once", 6, 0)[0][0][p] == 1   # found once per strand at the same place: one locus
    assert U.expected("palindrome_twice", 6, 0)[0][0][p] == 2
    three = U.expected("three_contigs", 35, 0)
    assert not three[1][0].any() and (three[2][0] > 0).sum() == 1  # shorter than k: no valid start; exactly k: one
    amb = U.expected("ambiguous", 16, 0)[0][0]
    assert not amb[85:103].any() and amb[40] >= 1               # starts over the drawn run are invalid; lower case is valid


@pytest.mark.parametrize("k,e", [(35, 0), (35, 1), (255, 0), (2, 1)])
def test_windows_equal_the_slices_of_the_whole(k, e):
    index, seq = U.case_index("planted"), _seqs("planted")[0]
    counts, cover = U.expected("planted", k, e)[0]
    for start, n in U.WINDOWS:
        wc, wv = mapad_amd.mappability_host(index, 0, seq, start=start, n=n, k=k, e=e)
        assert wc.tobytes() == counts[start:start + n].tobytes() and wv.tobytes() == cover[start:start + n].tobytes(), (start, n)
    only_counts, none = mapad_amd.mappability_host(index, 0, seq, start=37, n=101, k=k, e=e, cover=False)
    assert none is None and only_counts.tobytes() == counts[37:138].tobytes()
    none, only_cover = mapad_amd.mappability_host(index, 0, seq, start=37, n=101, k=k, e=e, counts=False)
    assert none is None and only_cover.tobytes() == cover[37:138].tobytes()


@pytest.mark.parametrize("k,e", [(16, 0), (35, 0), (35, 1)])
def test_verify_refuses_another_sequence(k, e):
    index = U.case_index("planted")
    other = U.rand_seq(300, 99).encode()
    with pytest.raises(mapad_amd.MapadError) as err:
        mapad_amd.mappability_host(index, 0, other, k=k, e=e, verify=True)
    assert err.value.code == -1
    with pytest.raises(mapad_amd.MapadError):
        mapad_amd.mappability_summary_host(index, [other], k=k, e=e, verify=True)


def test_errors():
    index, seq = U.case_index("planted"), _seqs("planted")[0]
    bad = [dict(k=0), dict(k=256), dict(e=2), dict(tid=1), dict(start=250, n=51), dict(start=301, n=0), dict(seq=seq[:-1]), dict(seq=seq + b"A")]
    for kw in bad:
        args = dict(tid=0, seq=seq, start=0, n=10, k=35, e=0)
        args.update(kw)
        with pytest.raises(mapad_amd.MapadError) as err:
            mapad_amd.mappability_host(index, args.pop("tid"), args.pop("seq"), **args)
        assert err.value.code == -1, kw
    for kw in (dict(k=0), dict(k=256), dict(e=2)):
        with pytest.raises(mapad_amd.MapadError):
            mapad_amd.mappability_summary_host(index, [seq], **kw)
    with pytest.raises(mapad_amd.MapadError):
        mapad_amd.mappability_summary_host(index, [seq[:-1]])


def _cli():
    from mapad_amd import build as b
    return b.build_cli()


@pytest.mark.parametrize("name,k,e", [("planted", 35, 0), ("planted", 16, 1), ("three_contigs", 35, 1), ("ambiguous", 16, 0)])
def test_cli_host_writes_what_the_rule_says(tmp_path, name, k, e):
    fasta = tmp_path / "ref.fa"
    U.write_reference(name, fasta)
    got = U.run_cli_files(_cli(), fasta, tmp_path, k, e, extra=("--host", "--verify"))
    want = U.expected_files(name, k, e)
    for key in want:
        assert got[key] == want[key], key
    assert want["start"] and want["bedgraph"]


def test_cli_refuses_bad_options_and_a_foreign_fasta(tmp_path):
    fasta = tmp_path / "ref.fa"
    U.write_reference("planted", fasta)
    for extra in (["-k", "0"], ["-k", "256"], ["--max_mismatches", "2"], ["--bed_rule", "most"]):
        r = subprocess.run([_cli(), "mappability", "-g", str(fasta), "--host", "--bed", str(tmp_path / "x.bed"), *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "mappability" in r.stderr, extra
    with open(fasta, "w") as f:  # same length, another sequence, the index stays
        f.write(">chrP\n" + U.rand_seq(300, 98) + "\n")
    r = subprocess.run([_cli(), "mappability", "-g", str(fasta), "--host", "--verify", "--bed", str(tmp_path / "x.bed")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--verify" in r.stderr
