"""The chunked part of the GPU index builder's prefix doubling (csrc/index_gpu.hip, step 3): the cut of the unresolved-row list at a group boundary (last head within the
chunk limit, else the first head behind it, else the tail), chunks larger than the limit, the still-tied rows of several chunks appended to one list, and the collection of
the unresolved rows in pieces.  With the limits of a real build (2^28 rows per chunk, 2^30 elements per sort) only a text with more than 2.7e8 tied suffixes — a genome
with its N runs — gets there; MAPAD_INDEX_DBL_CHUNK / MAPAD_INDEX_SORT_CAP lower them for one build, so texts of 10^5 symbols do.  Every index is held to the host SA-IS
build and to the numpy restatement of tests/index_util.py, and Index.last_build_info() proves which paths ran."""
import math

import numpy as np
import pytest

import mapad_amd
from mapad_amd import synth
from oracle import binding as ob

import index_util as iu
from kat_util import resolve_params
from parity_util import NO_DAMAGE, assert_same_as_oracle, split_reads
from test_gpu_index import assert_same_index

pytestmark = pytest.mark.gpu

COUNTERS = ("rounds", "unresolved", "chunks", "cut_last_head", "cut_first_head", "tails", "whole", "largest_chunk", "pieces")
# (text, rows per chunk, elements per sort, kinds of chunk end that a CPU simulation of the loop found for this setting, largest chunk exceeds the limit)
#   257 on two_copies_20k: every group is a pair, an odd limit falls inside one;  4097 on polyA / tandem: groups of n/2 and n/8 rows, far beyond the limit
SETTINGS = [
    ("mixed", 1000, 8192, ("cut_last_head", "cut_first_head", "tails", "whole"), True),
    ("mixed", 257, 8192, ("cut_last_head", "cut_first_head", "tails", "whole"), True),
    ("two_copies_20k", 257, 8192, ("cut_last_head",), False),
    ("n_runs", 1000, 32768, ("cut_last_head", "tails"), True),
    ("polyA", 4097, 1 << 20, ("cut_first_head", "tails"), True),
    ("tandem", 4097, 1 << 20, ("cut_first_head", "tails"), True),
]
IDS = [f"{s[0]}-{s[1]}-{s[2]}" for s in SETTINGS]

_built = {}  # (text, chunk, cap) -> (index, info): every setting is built once per process
_host = {}


def host_index(name):
    if name not in _host:
        _host[name] = mapad_amd.Index.build(iu.contigs(name))
    return _host[name]


def set_limits(monkeypatch, chunk, cap):
    for var, v in (("MAPAD_INDEX_DBL_CHUNK", chunk), ("MAPAD_INDEX_SORT_CAP", cap)):
        if v is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(v))


def built(monkeypatch, name, chunk, cap):
    key = (name, chunk, cap)
    if key not in _built:
        set_limits(monkeypatch, chunk, cap)
        ix = mapad_amd.Index.build(iu.contigs(name), device=0)
        _built[key] = (ix, mapad_amd.Index.last_build_info())
    return _built[key]


@pytest.mark.parametrize("name,chunk,cap,kinds,exceeds", SETTINGS, ids=IDS)
def test_chunked_doubling_equals_host_and_numpy_reference(name, chunk, cap, kinds, exceeds, monkeypatch):
    dev, info = built(monkeypatch, name, chunk, cap)
    print(f"\n{name} {chunk}/{cap}: {info}")
    assert_same_index(host_index(name), dev)
    iu.assert_index_equals_reference(dev, iu.reference(name), name)  # BWT, samples, extra rows, less, sentinels, and the SA of every row
    assert info["chunk_limit"] == chunk and info["sort_cap"] == cap
    for kind in kinds:
        assert info[kind] >= 1, (kind, info)
    if exceeds:
        assert info["largest_chunk"] > chunk, info
    assert info["rounds"] >= 2
    assert info["pieces"] == math.ceil(len(dev) / cap)
    assert info["unresolved"] > chunk  # the setting does cut
    assert info["chunks"] == info["cut_last_head"] + info["cut_first_head"] + info["tails"] + info["whole"]  # every chunk ends in exactly one of the four ways


def test_every_path_of_the_cut_ran(monkeypatch):
    """Over all settings together no counter stays zero: the condition that keeps this file from passing without running the code it is about."""
    infos = [built(monkeypatch, name, chunk, cap)[1] for name, chunk, cap, _, _ in SETTINGS]
    for c in COUNTERS:
        assert any(i[c] > 0 for i in infos), c
    assert any(i["largest_chunk"] > i["chunk_limit"] for i in infos)
    assert any(i["pieces"] > 1 for i in infos)


def test_defaults_build_in_one_chunk_per_round(monkeypatch):
    set_limits(monkeypatch, None, None)
    dev = mapad_amd.Index.build(iu.contigs("mixed"), device=0)
    info = mapad_amd.Index.last_build_info()
    assert info["chunk_limit"] == 1 << 28 and info["sort_cap"] == 1 << 30
    assert info["cut_last_head"] == info["cut_first_head"] == info["tails"] == 0
    assert info["rounds"] >= 2 and info["chunks"] == info["whole"] == info["rounds"] and info["pieces"] == 1
    assert info["largest_chunk"] == info["unresolved"]
    assert_same_index(host_index("mixed"), dev)
    for chunk in (1000, 257):
        ix, knob_info = built(monkeypatch, "mixed", chunk, 8192)
        assert_same_index(dev, ix)
        assert knob_info["unresolved"] == info["unresolved"]  # the same rows entered step 3, whatever the piece size of their collection


@pytest.mark.parametrize("name,chunk,cap,code,word", [
    ("polyA", 1000, 8192, -9, "prefix bucket holds more than 8192"),  # a bucket of 69 997 suffixes: beyond the sort call (MAPAD_ERR_UNSUPPORTED)
    ("uniform4097", 4096, 4096, -4, "MAPAD_INDEX_DBL_CHUNK"),         # chunk == cap: the search behind the limit would have nothing to look at
    ("uniform4097", 63, 8192, -4, "MAPAD_INDEX_DBL_CHUNK"),
    ("uniform4097", (1 << 28) + 1, 1 << 30, -4, "MAPAD_INDEX_DBL_CHUNK"),
    ("uniform4097", 1000, (1 << 30) + 1, -4, "MAPAD_INDEX_SORT_CAP"),
    ("uniform4097", 1000, "8k", -4, "MAPAD_INDEX_SORT_CAP"),
    ("uniform4097", -5, None, -4, "MAPAD_INDEX_DBL_CHUNK"),
], ids=["bucket_beyond_cap", "chunk_eq_cap", "chunk_63", "chunk_above_2^28", "cap_above_2^30", "cap_not_a_number", "chunk_negative"])
def test_limits_refuse_cleanly(name, chunk, cap, code, word, monkeypatch, capfd):
    """Host exceptions before any launch of step 2: the build returns an error, says which limit, and the next build in the process is unharmed."""
    set_limits(monkeypatch, chunk, cap)
    with pytest.raises(mapad_amd.MapadError) as e:
        mapad_amd.Index.build(iu.contigs(name), device=0)
    assert e.value.code == code
    assert word in capfd.readouterr().err
    set_limits(monkeypatch, None, None)
    dev = mapad_amd.Index.build(iu.contigs("uniform257"), device=0)
    assert_same_index(host_index("uniform257"), dev)
    iu.assert_index_equals_reference(dev, iu.reference("uniform257"), "uniform257")


def test_reads_map_on_an_index_built_through_the_cuts(monkeypatch):
    """200 reads of 40 bp from the unique part and from the 37 bp tandem of `mixed`, on the index built with 257 rows per chunk, bit for bit against the oracle."""
    pidx, info = built(monkeypatch, "mixed", 257, 8192)
    assert info["cut_last_head"] and info["cut_first_head"]
    text = np.frombuffer(b"".join(s for _, s in iu.contigs("mixed")), dtype=np.uint8)
    seqs, quals, offsets = synth.reads(text[:15_000 + 37 * 400], 200, 40, seed=77, qual=40)  # `mix` + the repeat of `u`: A, C, G, T only
    rp = resolve_params(NO_DAMAGE)
    ctx = mapad_amd.Context(pidx, mapad_amd.make_params(rp), 0)
    res = ctx.map_batch(seqs, quals, offsets)
    ctx.close()
    n_hits = np.diff(res.hit_begin.astype(np.int64))
    assert (n_hits > 0).sum() > 150 and len(n_hits) == 200  # 10 % of synth's reads are random sequence
    assert (res.hits_arr["size"] > 100).any() and (res.hits_arr["size"] == 1).any()  # reads from the tandem (some 400 rows each) and from the unique part
    oidx = ob.OracleIndex.from_bwt(iu.reference("mixed").bwt, "$ACGTX", 128)  # the oracle's own structures over the numpy reference's BWT
    reads, qs = split_reads(seqs, quals, offsets)
    ores = oidx.map_batch(ob.make_params(rp), reads, qs, n_threads=8, keep_d=True)
    assert_same_as_oracle(ores, res, offsets)
