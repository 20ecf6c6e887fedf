"""Quality rescaling on the GPU (run with -m gpu on an MI355X): what rescale_kernel writes while batches are converted to records — the batch's qualities with the
likely-damaged bases marked down, the context's summary, and in mode 2 what the pileup's base-quality filter sees — equals mapad_quality_rescale_host over the
same fetched results and seeds bit for bit, under every path a batch can take (both search steps, one quality level, duplicate collapsing, the host tail,
batches in flight, the CLI), and equals the qualities decoded independently from the records / the BAM (tests/rescale_util.py)."""
import subprocess

import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd import build as mbuild
from mapad_amd import synth

import damage_util as du
import pileup_util as pu
import rescale_util as ru
from bam_util import read_bam
from kat_util import resolve_params
from parity_util import DAMAGE, DOUBLE_STRANDED, IGNORE_BQ

pytestmark = pytest.mark.gpu

DMG = dict(f=0.5, t=0.5, d=0.02, s=1.0)
SEED = 99
# TestDifferenceModel + TestBound: the alignment starts in the middle of the read, so the general-direction search step runs and the operations of a track are not
# in read order
TEST_MODEL = {"model": "test", "deam_score": -0.5, "mm_score": -1.0, "match_score": 0.0, "bound": "test", "threshold": -2.0, "repr_mm_bound": -1.0,
              "penalty_gap_open": -2.0, "penalty_gap_extend": -1.0, "gap_dist_ends": 5, "max_num_gaps_open": 1}
MODELS = {"ss": DAMAGE, "ds": DOUBLE_STRANDED, "test_model": TEST_MODEL, "ignore_bq": IGNORE_BQ}
GUARD = ["timeout", "-k", "10", "300"]  # every GPU child process under a time limit of its own
SPLIT = 250_000
LENGTHS = [SPLIT, 400_000 - SPLIT]


@pytest.fixture(scope="module")
def world():
    g = synth.genome(400_000, seed=77)
    g[300_000:300_400] = g[100_000:100_400]  # a repeat: reads from it have X0 > 1
    return g, mapad_amd.Index.build([("c1", g[:SPLIT]), ("c2", g[SPLIT:])])


def mixed_batch(g, n, seed):
    a = synth.reads(g, n, seed=seed, qual_range=(20, 40), damage=DMG, len_range=(20, 70), indel_frac=0.2)
    b = synth.reads(g[100_000:100_400], n // 10, 45, seed=seed + 1, exo_frac=0.0, damage=DMG)
    seqs, quals, offsets = pu.concat(a, b)
    quals = quals.copy()
    quals[::97] = 255  # missing qualities, 0 and 93 among the usual ones
    quals[1::101] = 0
    quals[2::103] = 93
    return seqs, quals, offsets


def seed_at(first_read):
    return int(mapad_amd.lib().mapad_records_seed_at(SEED, first_read))


def convert(ctx, res, batch, seed=SEED):
    """records on the device (which rescales the batch) -> the rescaled qualities"""
    out = ctx.hits_to_records(res, *batch, seed=seed, as_arrays=True, rescaled=True)
    assert len(out) == 3 and out[2] is not None, "the records carry no rescaled qualities"
    assert len(ctx.hits_to_records(res, *batch, seed=seed, as_arrays=True)) == 2  # without the keyword: the shape of today
    return out[2]


def assert_same(got, want, what=""):
    """(rescaled qualities, summary) of the device against the host path's: everything but kernel_ms"""
    assert got[0].dtype == np.uint8 and got[0].shape == want[0].shape, what
    assert np.array_equal(got[0], want[0]), (what, np.flatnonzero(got[0] != want[0])[:10])
    ru.assert_summary(got[1], want[1], what)


@pytest.mark.parametrize("model", list(MODELS))
def test_device_bytes_equal_the_host_path(world, model):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(MODELS[model]))
    batch = mixed_batch(g, 4000, seed=5)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_quality_rescale(1)
        res = ctx.map_batch(*batch)
        out = convert(ctx, res, batch)
        recs, again = ctx.hits_to_records(res, *batch, seed=SEED, rescaled=True)  # the same batch again, as dicts: the same bytes, nothing added
        got = ctx.quality_rescale()
    finally:
        ctx.close()
    want = mb.quality_rescale_host(idx, params, res, *batch, seed=SEED)
    assert_same((out, got), want, model)
    assert np.array_equal(again, out)
    seqs, quals, offsets = batch
    n = len(offsets) - 1
    assert got["batches"] == 1 and got["reads_seen"] == n and 0 < got["reads_rescaled"] < n and got["kernel_ms"] > 0.0
    changed = out != quals
    assert 0 < changed.sum() < got["candidate_columns"].sum() and changed.sum() == got["bases_changed"]  # some bytes change, not every candidate (Q0, Q255)
    assert changed.sum() < 0.05 * len(quals) and (out <= quals).all() and (out[quals == 255] == 255).all()
    dq, dsum = ru.from_records(params, recs, batch)  # and the qualities decoded from the device's records in plain Python
    assert_same((out, got), (dq, dsum), model + ": decoded from the records")


def _planted(g, n, reverse, quals_at_ends, start):
    """a read of n bases with a C->T planted at read positions 0 and n - 1 (in read orientation; `reverse`: the read is the reverse complement of the genome
    there), the given quality bytes on those two columns"""
    want = ord("G") if reverse else ord("C")
    at = start
    while not (g[at] == want and g[at + n - 1] == want):
        at += 1
    r = g[at:at + n].copy()
    if reverse:
        r = synth.revcomp(r)
    assert r[0] == ord("C") and r[-1] == ord("C")
    r[0] = r[-1] = ord("T")
    q = np.full(n, 30, np.uint8)
    q[0], q[-1] = quals_at_ends
    return r, q


def _batch_of(pairs):
    offs = np.zeros(len(pairs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r, _ in pairs])
    return np.concatenate([r for r, _ in pairs]).astype(np.uint8), np.concatenate([q for _, q in pairs]).astype(np.uint8), offs


def test_smallest_batches_tracks_at_the_trip_boundaries_and_planted_columns(world):
    """one read; five reads (not a multiple of the block's four wavefronts); a batch with no mapped read; tracks of 63, 64, 65 and 129 operations (trips of 64 lanes);
    a C->T planted at read positions 0 and L - 1, forward and reverse-complemented, with quality bytes 0, 30, 93 and 255 on those columns"""
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    rng = np.random.Generator(np.random.PCG64(3))
    acgt = np.frombuffer(b"ACGT", np.uint8)
    ends = [(30, 30), (0, 93), (93, 0), (255, 30), (30, 255)]
    trips = [_planted(g, n, rev, ends[k % 5], 20_000 + 700 * k) for k, (n, rev) in enumerate([(n, rev) for rev in (False, True) for n in (63, 64, 65, 129)] + [(129, False), (64, True)])]
    batches = {"one": _batch_of([_planted(g, 50, False, (30, 30), 10_000)]),
               "five": _batch_of([_planted(g, 40 + k, k % 2 == 1, ends[k], 11_000 + 200 * k) for k in range(5)]),
               "unmapped": pu.hand_made([acgt[rng.integers(0, 4, 50)] for _ in range(6)]), "trips": _batch_of(trips),
               "one_again": _batch_of([_planted(g, 33, True, (93, 93), 12_000)])}
    tab = {L: mapad_amd.quality_rescale_table(params, L) for L in (33, 50, 63, 64, 65, 129) + tuple(range(40, 45))}
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_quality_rescale(1)
        want_sum, first = None, 0
        for name, batch in batches.items():
            seqs, quals, offsets = batch
            res = ctx.map_batch(*batch)
            out = convert(ctx, res, batch, seed=seed_at(first))
            recs = ctx.hits_to_records(res, *batch, seed=seed_at(first))
            want, want_sum = mb.quality_rescale_host(idx, params, res, *batch, seed=seed_at(first), into=want_sum)
            assert np.array_equal(out, want), name
            k = len(offsets) - 1
            if name == "unmapped":
                assert not any(r["mapped"] for r in recs) and np.array_equal(out, quals)  # the bytes come back unchanged
            else:
                assert all(r["mapped"] for r in recs), name
                for r in range(k):  # exactly the two planted columns changed, each to its table entry (Q0 and the missing quality stay)
                    a, b = int(offsets[r]), int(offsets[r + 1])
                    L = b - a
                    assert recs[r]["cigar"] == "%dM" % L and recs[r]["nm"] == 2, (name, r, recs[r])
                    exp = quals[a:b].copy()
                    for p in (0, L - 1):
                        if exp[p] != 255:
                            exp[p] = tab[L][p, int(exp[p]), 0]
                    assert np.array_equal(out[a:b], exp), (name, r)
                    assert all(out[a + p] < quals[a + p] for p in (0, L - 1) if quals[a + p] not in (0, 255)), (name, r)
            if name == "trips":
                assert [r["reverse"] for r in recs] == [False] * 4 + [True] * 4 + [False, True]
            first += k
        got = ctx.quality_rescale()
    finally:
        ctx.close()
    ru.assert_summary(got, want_sum, "five small batches")
    assert got["batches"] == 5 and got["reads_seen"] == first and got["reads_rescaled"] == first - 6 and got["candidate_columns"][0] == 2 * (first - 6)


def test_collapsing_and_the_host_tail_change_no_byte(world, monkeypatch):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = du.with_duplicates(mixed_batch(g, 2000, seed=15), 1500, seed=3)
    want = mb.quality_rescale_host  # (called per result below: every result is its own fetch)
    got = {}
    for collapse in (True, False):
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_collapse_duplicates(collapse)
            ctx.set_quality_rescale(1)
            res = ctx.map_batch(*batch)
            if collapse:
                info = ctx.collapse_info()
                assert info[1] < info[0] == len(batch[2]) - 1
            got[collapse] = (convert(ctx, res, batch), ctx.quality_rescale())
            assert_same(got[collapse], want(idx, params, res, *batch, seed=SEED), f"collapse={collapse}")
        finally:
            ctx.close()
    assert_same(got[True], got[False], "collapsed against not collapsed")
    monkeypatch.setenv("MAPAD_TAIL_BACKLOG_BUDGET", "4294967295")  # every read past the budget leaves for the host
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_tail_pops(48)
        ctx.set_quality_rescale(1)
        res = ctx.map_batch(*batch)
        assert ctx.tail_info()["reads"] > 100
        tail = (convert(ctx, res, batch), ctx.quality_rescale())
    finally:
        ctx.close()
    assert_same(tail, want(idx, params, res, *batch, seed=SEED), "host tail")
    assert_same(tail, got[False], "host tail against the GPU alone")


def test_batches_in_flight_and_a_batch_converted_twice(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batches = [mixed_batch(g, 1000 + 300 * k, seed=40 + k) for k in range(5)]
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_pipeline_depth(3)
        ctx.set_quality_rescale(1)
        want, flying, first = None, [], 0
        todo = list(batches)
        while todo or flying:
            while todo and len(flying) < 3:
                ctx.submit_batch(*todo[0])
                flying.append(todo.pop(0))
            ctx.select_batch(len(flying) - 1)  # the oldest
            b = flying.pop(0)
            res = ctx.fetch()
            out = convert(ctx, res, b, seed=seed_at(first))
            w, want = mb.quality_rescale_host(idx, params, res, *b, seed=seed_at(first), into=want)
            assert np.array_equal(out, w)
            first += len(b[2]) - 1
        got = ctx.quality_rescale()
        ru.assert_summary(got, want, "five batches, three in flight")
        assert got["batches"] == 5 and got["reads_seen"] == first
        # the last batch, still resident: converted again and through mapad_records_device it returns the same bytes and adds nothing
        again = convert(ctx, res, b, seed=seed_at(first - (len(b[2]) - 1)))
        ctx.records_device(seed=SEED)
        assert np.array_equal(again, out)
        ru.assert_summary(ctx.quality_rescale(), got, "converted twice")
        assert ctx.quality_rescale()["batches"] == 5
        ctx.reset_quality_rescale()
        zero = ctx.quality_rescale()
        assert zero["batches"] == 0 and zero["reads_seen"] == 0 and zero["bases_changed"] == 0 and not zero["new_quality"].any() and not zero["candidate_columns"].any()
        assert zero["kernel_ms"] == 0.0
    finally:
        ctx.close()


def test_mode_2_feeds_the_pileup_filter_and_mode_1_does_not(world):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 3000, seed=55)
    flt = (25, 0, 0)  # min_base_quality = 25
    got = {}
    for mode in (1, 2):
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            ctx.set_pileup(1, *flt)
            ctx.set_quality_rescale(mode)
            res = ctx.map_batch(*batch)
            out = convert(ctx, res, batch)
            got[mode] = (ctx.pileup(3, 80), [ctx.pileup_counts(t, 0, n) for t, n in enumerate(LENGTHS)], out, res)
        finally:
            ctx.close()
    assert np.array_equal(got[1][2], got[2][2])  # the same bytes travel with the records under both modes
    seqs, quals, offsets = batch
    host_q, _ = mb.quality_rescale_host(idx, params, got[2][3], *batch, seed=SEED)
    assert np.array_equal(host_q, got[2][2])
    for mode, q in ((1, quals), (2, host_q)):  # mode 1: today's pileup; mode 2: the pileup of the host-rescaled qualities
        p, pc, _, res = got[mode]
        pil = mb.PileupHost(idx, 1, *flt).add(params, res, seqs, q, offsets, seed=SEED)
        pu.assert_equal(p, pil.summary(3, 80), 3, 80, "pileup under rescale mode %d against the host path" % mode)
        for t, n in enumerate(LENGTHS):
            assert np.array_equal(pc[t], pil.counts(t, 0, n)), (mode, t)
    assert got[2][0]["columns_low_quality"] > got[1][0]["columns_low_quality"] and got[2][0]["columns_counted"] < got[1][0]["columns_counted"]
    assert any(not np.array_equal(a, b) for a, b in zip(got[1][1], got[2][1]))


def _record_texts(recs, text):
    """the CIGAR, MD and XA bytes of every record, in record order"""
    blob = text.tobytes()
    return [tuple(blob[int(r[k + "_off"]):int(r[k + "_off"]) + int(r[k + "_len"])] for k in ("cigar", "md", "xa")) for r in recs]


def _assert_same_records(a, b, same_pool):
    """every field of every record and the CIGAR, MD and XA bytes its offsets point to.  Pool offsets only on the host text path (same_pool): the device text
    pool is filled in arrival order."""
    assert len(a[0]) == len(b[0]) and _record_texts(a[0], a[1]) == _record_texts(b[0], b[1])
    for k in a[0].dtype.names:
        if k and not k.startswith("_") and (same_pool or not k.endswith("_off")):
            assert np.array_equal(a[0][k], b[0][k]), k
    if same_pool:
        assert a[1].tobytes() == b[1].tobytes()


def test_off_is_off_and_uploaded_hits_are_refused_only_while_on(world, monkeypatch):
    g, idx = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = mixed_batch(g, 1500, seed=65)
    fresh, a, b = mapad_amd.Context(idx, params, 0), mapad_amd.Context(idx, params, 0), mapad_amd.Context(idx, params, 0)

    def both_paths(ctx, res):
        out = {"device": ctx.hits_to_records(res, *batch, seed=SEED, as_arrays=True, rescaled=True)}
        with monkeypatch.context() as m:
            m.setenv("MAPAD_RECORDS_TEXT", "host")  # read at every records call
            out["host"] = ctx.hits_to_records(res, *batch, seed=SEED, as_arrays=True, rescaled=True)
        return out

    try:
        want = both_paths(fresh, fresh.map_batch(*batch))
        assert all(len(v) == 3 and v[2] is None for v in want.values())  # no qualities beside the records
        never = fresh.quality_rescale()
        assert never["batches"] == 0 and never["reads_seen"] == 0 and not never["new_quality"].any()
        a.set_quality_rescale(2)
        res_on = a.map_batch(*batch)
        on = both_paths(a, res_on)  # both records paths carry the same bytes
        assert all(len(v) == 3 for v in on.values()) and np.array_equal(on["device"][2], on["host"][2])
        assert_same((on["host"][2], a.quality_rescale()), mb.quality_rescale_host(idx, params, res_on, *batch, seed=SEED), "host text path")
        assert (on["host"][2] != batch[1]).any()
        _assert_same_records(on["device"], want["device"], same_pool=False)  # the rescaling changes no record
        _assert_same_records(on["host"], want["host"], same_pool=True)
        a.set_quality_rescale(0)
        off = both_paths(a, a.map_batch(*batch))
        assert all(len(v) == 3 and v[2] is None for v in off.values())  # mapad_records_rescaled_quals returns NULL
        _assert_same_records(off["device"], want["device"], same_pool=False)
        _assert_same_records(off["host"], want["host"], same_pool=True)
        assert a.quality_rescale()["batches"] == 0
        recs, none = a.hits_to_records(res_on, *batch, seed=SEED, rescaled=True)
        assert none is None and recs == a.hits_to_records(res_on, *batch, seed=SEED)
        # another context's result: its hits are uploaded
        plain = fresh.hits_to_records(res_on, *batch, seed=SEED)
        assert b.hits_to_records(res_on, *batch, seed=SEED) == plain
        b.set_quality_rescale(1)
        with pytest.raises(mapad_amd.MapadError) as e:
            b.hits_to_records(res_on, *batch, seed=SEED)
        assert e.value.code == -9  # MAPAD_ERR_UNSUPPORTED
        assert b.quality_rescale()["batches"] == 0
        b.set_quality_rescale(0)
        assert b.hits_to_records(res_on, *batch, seed=SEED) == plain
        for bad in (3, -1):
            with pytest.raises(mapad_amd.MapadError) as e:
                a.set_quality_rescale(bad)
            assert e.value.code == -1
        with monkeypatch.context() as m:  # MAPAD_RESCALE sets the default of new contexts
            m.setenv("MAPAD_RESCALE", "1")
            c = mapad_amd.Context(idx, params, 0)
        try:
            by_env = c.hits_to_records(c.map_batch(*batch), *batch, seed=SEED, as_arrays=True, rescaled=True)[2]
            assert np.array_equal(by_env, on["device"][2]) and c.quality_rescale()["batches"] == 1
        finally:
            c.close()
    finally:
        fresh.close()
        a.close()
        b.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def _read_report(path):
    lines = open(path).read().splitlines()
    head = dict(kv.split("=") for kv in lines[0].split()[2:])
    assert lines[0].startswith("#mapad-amd-rescale v1 ") and head["bins"] == "64"
    assert lines[1] == "#reads_seen\treads_rescaled\tcandidate_ct\tcandidate_ga\tbases_changed\tquality_drop_sum\tbatches" and lines[3] == "#new_quality\tbases" and len(lines) == 4 + 64
    v = [int(x) for x in lines[2].split("\t")]
    d = dict(reads_seen=v[0], reads_rescaled=v[1], candidate_columns=np.array(v[2:4], np.uint64), bases_changed=v[4], quality_drop_sum=v[5], batches=v[6])
    rows = [ln.split("\t") for ln in lines[4:]]
    assert [int(r[0]) for r in rows] == list(range(64))
    d["new_quality"] = np.array([int(r[1]) for r in rows], np.uint64)
    return head, d


def test_cli_writes_the_rescaled_qualities_into_the_bam(tmp_path):
    """QUAL of every record of `mapad-amd map --rescale_qualities` equals the array Python gets for the same reads (reversed for reverse-strand records like the
    input's), unmapped records are untouched; OQ:Z is present exactly where QUAL changed, equals the input and replaces an input OQ; without the flag QUAL is
    the input's and there is no OQ; the report equals Context.quality_rescale(); --rescale_pileup without --pileup is refused."""
    from bam_util import write_bam
    mapad_amd.lib()
    cli = mbuild.build_cli()
    g = synth.genome(120_000, seed=17)
    fa, fq = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fastq")
    with open(fa, "w") as f:
        f.write(">chr1\n")
        s = g.tobytes().decode()
        for i in range(0, len(s), 60):
            f.write(s[i:i + 60] + "\n")
    seqs, quals, offsets = synth.reads(g, 2500, seed=23, qual_range=(20, 40), damage=DMG, len_range=(25, 80), indel_frac=0.2)
    quals = quals.copy()
    quals[1::101] = 0
    quals[2::103] = 93
    batch = (seqs, quals, offsets)
    n = len(offsets) - 1
    phred = lambda q: "".join(chr(33 + int(x)) for x in q)  # noqa: E731
    with open(fq, "w") as f:
        for i in range(n):
            s, e = int(offsets[i]), int(offsets[i + 1])
            f.write(f"@r{i}\n{seqs[s:e].tobytes().decode()}\n+\n{phred(quals[s:e])}\n")
    subprocess.check_call(GUARD + [cli, "index", "-g", fa])
    model = ["-g", fa, "-l", "single_stranded", "-p", "0.03", "-f", "0.5", "-t", "0.5", "-d", "0.02", "-s", "1.0", "-i", "0.001", "--seed", "7", "--batch_size", "1000"]
    base = GUARD + [cli, "map", "-r", fq] + model
    params = mapad_amd.params_from_cli(library="single_stranded", five_prime_overhang=0.5, three_prime_overhang=0.5, ds_deamination_rate=0.02, ss_deamination_rate=1.0,
                                       poisson_prob=0.03, indel_rate=0.001)
    idx = mapad_amd.Index.build([("chr1", g)])
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        ctx.set_quality_rescale(1)
        res = ctx.map_batch(*batch)
        want_q = convert(ctx, res, batch, seed=7)
        want = ctx.quality_rescale()
    finally:
        ctx.close()

    def check(recs, inputs_oq):
        """QUAL is the Python-side array, with orientation; OQ (inputs_oq: it was asked for) exactly where QUAL changed, equal to the input"""
        assert len(recs) == n
        changed_records = 0
        for i, r in enumerate(recs):
            a, b = int(offsets[i]), int(offsets[i + 1])
            rev = bool(r["flags"] & 0x10)
            orient = (lambda q: q[::-1]) if rev else (lambda q: q)
            if r["flags"] & 0x4:
                assert r["qual"] == phred(quals[a:b]) and "OQ" not in r["tags"], i  # unmapped: untouched
                continue
            assert r["qual"] == phred(orient(want_q[a:b])), i
            changed = bool((want_q[a:b] != quals[a:b]).any())
            changed_records += changed
            assert ("OQ" in r["tags"]) == (changed and inputs_oq), i
            if changed and inputs_oq:
                assert r["tags"]["OQ"] == ("Z", phred(orient(quals[a:b]))) and r["tag_order"].count("OQ") == 1, i
                assert r["tag_order"][-1] == "OQ"  # behind everything else, DS included
        assert 0 < changed_records < n
        return changed_records

    pil = {name: str(tmp_path / f"pileup_{name}.tsv") for name in ("raw", "rescaled")}
    plain_bam = str(tmp_path / "plain.bam")
    pr = subprocess.run(base + ["-o", plain_bam, "--pileup", pil["raw"], "--pileup_min_bq", "25"], check=True, stderr=subprocess.PIPE, text=True)
    assert "quality rescaling" not in pr.stderr
    for i, r in enumerate(read_bam(plain_bam)[2]):  # without the flag: no OQ, QUAL equal to the input
        q = phred(quals[int(offsets[i]):int(offsets[i + 1])])
        assert "OQ" not in r["tags"] and r["qual"] == (q[::-1] if r["flags"] & 0x10 else q), i
    # the rescaled QUAL, the report, and OQ behind DS in the tag order
    keep, tsv = str(tmp_path / "keep.bam"), str(tmp_path / "rescaled.tsv")
    pr = subprocess.run(base + ["-o", keep, "--rescale_qualities", "--rescale_keep_original", "--damage_score", "--rescale_report", tsv], check=True, stderr=subprocess.PIPE, text=True)
    assert "quality rescaling (records)" in pr.stderr, pr.stderr
    recs = read_bam(keep)[2]
    check(recs, True)
    assert all(r["tag_order"][-2:] == ["DS", "OQ"] for r in recs if "OQ" in r["tags"])
    head, d = _read_report(tsv)
    assert head["mode"] == "records" and d["batches"] == 3
    ru.assert_summary(d, dict(want, batches=3), "the report")
    # an input OQ is replaced: the same reads from a BAM whose every record carries a wrong one
    bam_in, again = str(tmp_path / "in.bam"), str(tmp_path / "again.bam")
    write_bam(bam_in, "@HD\tVN:1.0\n", [], [{"name": f"r{i}", "flags": 4, "seq": seqs[int(offsets[i]):int(offsets[i + 1])].tobytes().decode(),
                                              "qual": phred(quals[int(offsets[i]):int(offsets[i + 1])]), "tags": [("OQ", "Z", "wrong")]} for i in range(n)])
    # ... in the run that also feeds the pileup's filter (mode 2): the same BAM, another pileup than the plain run's
    pr = subprocess.run(GUARD + [cli, "map", "-r", bam_in] + model + ["-o", again, "--rescale_qualities", "--rescale_keep_original", "--rescale_pileup", "--pileup", pil["rescaled"],
                                                                      "--pileup_min_bq", "25"], check=True, stderr=subprocess.PIPE, text=True)
    assert "quality rescaling (pileup)" in pr.stderr, pr.stderr
    check(read_bam(again)[2], True)
    assert open(pil["raw"]).read() != open(pil["rescaled"]).read()
    # --rescale_pileup is refused without a pileup, the other flags without --rescale_qualities (both before anything is mapped)
    pr = subprocess.run(base + ["-o", str(tmp_path / "no.bam"), "--rescale_qualities", "--rescale_pileup"], stderr=subprocess.PIPE, text=True)
    assert pr.returncode != 0 and "--rescale_pileup needs --pileup FILE or --consensus FASTA" in pr.stderr, pr.stderr
    pr = subprocess.run(base + ["-o", str(tmp_path / "no.bam"), "--rescale_keep_original"], stderr=subprocess.PIPE, text=True)
    assert pr.returncode != 0 and "need --rescale_qualities" in pr.stderr, pr.stderr
