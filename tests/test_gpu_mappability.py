"""The mappability stage on the GPU (run with -m gpu on an MI355X): mappability_count_kernel, mappability_cover_kernel and mappability_summary_kernel through
mapad_ctx_mappability, mapad_ctx_mappability_summary and `mapad-amd mappability`, byte for byte against the host path and the rule in plain Python
(tests/mappability_util.py), over the same case table as the host tests."""
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import build as mbuild
from mapad_amd import presets, synth

import mappability_util as U

pytestmark = pytest.mark.gpu

GUARD = ["timeout", "-k", "10", "120"]  # every GPU child process under a time limit of its own


def _params():
    return mapad_amd.make_params(presets.resolve(presets.DAMAGE))


def _seqs(name):
    return [s.encode() for _, s in U.CASES[name][0]]


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(name):
        if name not in made:
            made[name] = mapad_amd.Context(U.case_index(name), _params(), 0)
        return made[name]

    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("name,k,e", U.PARAMS)
def test_device_equals_host_equals_the_rule(contexts, name, k, e):
    ctx, index, exp = contexts(name), U.case_index(name), U.expected(name, k, e)
    for tid, seq in enumerate(_seqs(name)):
        counts, cover = ctx.mappability(tid, seq, k=k, e=e)
        hc, hv = mapad_amd.mappability_host(index, tid, seq, k=k, e=e)
        assert counts.tobytes() == hc.tobytes() == exp[tid][0].tobytes(), (tid, "counts")
        assert cover.tobytes() == hv.tobytes() == exp[tid][1].tobytes(), (tid, "cover")
        vc, vv = ctx.mappability(tid, seq, k=k, e=e, verify=True)  # the right sequence passes and changes nothing
        assert vc.tobytes() == counts.tobytes() and vv.tobytes() == cover.tobytes()
    got = ctx.mappability_summary(_seqs(name), k=k, e=e)
    host = mapad_amd.mappability_summary_host(index, _seqs(name), k=k, e=e)
    want = U.expected_figures(name, k, e)
    assert got["contigs"] == host["contigs"] and got["total"] == host["total"] == U.add_figures(want)
    assert [{key: c[key] for key in want[0]} for c in got["contigs"]] == want
    assert got["starts"] == host["starts"] == sum(len(s) for s in _seqs(name))
    assert got["steps"] == host["steps"] > 0  # the same chains, step for step


@pytest.mark.parametrize("k,e", [(35, 0), (35, 1), (255, 0), (2, 1)])
def test_tiles_and_windows(contexts, monkeypatch, k, e):
    ctx, seq = contexts("planted"), _seqs("planted")[0]
    counts, cover = U.expected("planted", k, e)[0]
    for tile in ("64", "1", "100"):  # 300 starts in several tiles, the cover's halo across them (k - 1 = 254 is longer than a tile of 64)
        if tile == "1" and e:
            continue
        monkeypatch.setenv("MAPAD_MAPPABILITY_TILE", tile)
        tc, tv = ctx.mappability(0, seq, k=k, e=e)
        assert tc.tobytes() == counts.tobytes() and tv.tobytes() == cover.tobytes(), tile
        for start, n in U.WINDOWS:
            wc, wv = ctx.mappability(0, seq, start=start, n=n, k=k, e=e)
            assert wc.tobytes() == counts[start:start + n].tobytes() and wv.tobytes() == cover[start:start + n].tobytes(), (tile, start, n)
        got = ctx.mappability_summary([seq], k=k, e=e)
        assert {key: got["total"][key] for key in ("valid_starts", "unique_starts", "hist", "majority", "strict")} == \
            {key: U.rule_figures(counts, cover, k)[key] for key in ("valid_starts", "unique_starts", "hist", "majority", "strict")}, tile
    monkeypatch.delenv("MAPAD_MAPPABILITY_TILE")
    for start, n in U.WINDOWS:
        wc, wv = ctx.mappability(0, seq, start=start, n=n, k=k, e=e)
        assert wc.tobytes() == counts[start:start + n].tobytes() and wv.tobytes() == cover[start:start + n].tobytes(), (start, n)
    only_counts, none = ctx.mappability(0, seq, start=37, n=101, k=k, e=e, cover=False)
    assert none is None and only_counts.tobytes() == counts[37:138].tobytes()
    none, only_cover = ctx.mappability(0, seq, start=37, n=101, k=k, e=e, counts=False)
    assert none is None and only_cover.tobytes() == cover[37:138].tobytes()


@pytest.mark.parametrize("value", ["0", "-3", "abc", "64x", str((1 << 22) + 1)])
def test_an_invalid_tile_is_a_parse_error(contexts, monkeypatch, value):
    monkeypatch.setenv("MAPAD_MAPPABILITY_TILE", value)
    with pytest.raises(mapad_amd.MapadError) as err:
        contexts("planted").mappability(0, _seqs("planted")[0])
    assert err.value.code == -4


@pytest.mark.parametrize("k,e", [(16, 0), (35, 0), (35, 1)])
def test_verify_refuses_another_sequence(contexts, k, e):
    ctx = contexts("planted")
    other = U.rand_seq(300, 99).encode()
    with pytest.raises(mapad_amd.MapadError) as err:
        ctx.mappability(0, other, k=k, e=e, verify=True)
    assert err.value.code == -1
    with pytest.raises(mapad_amd.MapadError):
        ctx.mappability_summary([other], k=k, e=e, verify=True)
    counts, _ = ctx.mappability(0, _seqs("planted")[0], k=k, e=e, verify=True)  # the context goes on working
    assert counts.tobytes() == U.expected("planted", k, e)[0][0].tobytes()


def test_errors(contexts):
    ctx, seq = contexts("planted"), _seqs("planted")[0]
    bad = [dict(k=0), dict(k=256), dict(e=2), dict(tid=1), dict(start=250, n=51), dict(start=301, n=0), dict(seq=seq[:-1]), dict(seq=seq + b"A")]
    for kw in bad:
        args = dict(tid=0, seq=seq, start=0, n=10, k=35, e=0)
        args.update(kw)
        with pytest.raises(mapad_amd.MapadError) as err:
            ctx.mappability(args.pop("tid"), args.pop("seq"), **args)
        assert err.value.code == -1, kw
    for kw in (dict(k=0), dict(k=256), dict(e=2)):
        with pytest.raises(mapad_amd.MapadError):
            ctx.mappability_summary([seq], **kw)
    with pytest.raises(mapad_amd.MapadError):
        ctx.mappability_summary([seq[:-1]])


def test_a_call_between_two_batches_leaves_them_alone():
    seq = _seqs("planted")[0]
    genome = np.frombuffer(seq, np.uint8).copy()
    index = U.case_index("planted")
    batches = [synth.reads(genome, 200, 50, seed=s, qual_range=(20, 40), damage=dict(f=0.5, t=0.5, d=0.02, s=1.0)) for s in (3, 4)]

    def run(with_call):
        ctx = mapad_amd.Context(index, _params(), 0)
        out = []
        for i, (seqs, quals, offsets) in enumerate(batches):
            res = ctx.map_batch(seqs, quals, offsets)
            out.append((res.hit_begin.copy(), res.hits_arr.copy(), res.ops.copy()))
            if with_call and i == 0:
                counts, cover = ctx.mappability(0, seq, k=35, e=1)
                assert counts.tobytes() == U.expected("planted", 35, 1)[0][0].tobytes() and cover.tobytes() == U.expected("planted", 35, 1)[0][1].tobytes()
        ctx.close()
        return out

    plain, mixed = run(False), run(True)
    assert int(np.diff(plain[1][0].astype(np.int64)).clip(0, 1).sum()) > 100  # reads do map here
    for a, b in zip(plain, mixed):
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("name,k,e,rule", [("planted", 35, 0, "strict"), ("planted", 16, 1, "majority"), ("three_contigs", 35, 1, "start"), ("ambiguous", 16, 0, "majority")])
def test_cli_writes_what_the_rule_says(tmp_path, name, k, e, rule):
    """(every BED rule on every case: the host tests — the runs are cut on the host by the same code)"""
    cli = mbuild.build_cli()
    fasta = tmp_path / "ref.fa"
    U.write_reference(name, fasta)
    want = U.expected_files(name, k, e)
    bed, bg, rep = (str(tmp_path / f"dev.{ext}") for ext in ("bed", "bedgraph", "tsv"))
    subprocess.run(GUARD + [cli, "mappability", "-g", str(fasta), "-k", str(k), "--max_mismatches", str(e), "--verify", "--bed", bed, "--bed_rule", rule, "--bedgraph", bg,
                            "--report", rep], check=True, capture_output=True, timeout=150)
    assert open(bed).read() == want[rule] and want[rule]
    assert open(bg).read() == want["bedgraph"] and open(rep).read() == want["report"]
