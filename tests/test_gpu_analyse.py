"""The accumulator stages over existing alignments on the GPU (run with -m gpu on an MI355X): the tracks align_count_kernel and align_build_kernel build equal the
host path's bit for bit; a context that is GIVEN the records another context mapped — contig, position, strand, CIGAR, MD, X0, AS — ends with every table,
summary, call, duplicate flag, score and rescaled quality of the context that mapped them; batch cuts do not matter; reads of any class but ok are seen, not
counted; the mapping-quality threshold equals leaving those reads out."""
import numpy as np
import pytest

import mapad_amd

import analyse_util as au
import damage_util as du
import panel_util as pn
from kat_util import resolve_params
from parity_util import DAMAGE
from test_gpu_panel import TEST_MODEL

pytestmark = pytest.mark.gpu

SEED = 99
MODELS = {"ss": DAMAGE, "test_model": TEST_MODEL}
LENGTHS = pn.LENGTHS
FILTER = (30, 3, 2)
RULE = dict(call=0, min_depth=1, transitions=2, seed=31)


@pytest.fixture(scope="module")
def world():
    g = pn.world_genome()
    return g, mapad_amd.Index.build([("c1", g[:pn.SPLIT]), ("c2", g[pn.SPLIT:])]), pn.panel(g)


def all_stages(ctx, p, mode):
    """the nine stages, every one in `mode` (2: X0 == 1 only, duplicates and low scores left out, rescaled qualities feed the filters)"""
    ctx.set_mark_duplicates(mode)
    ctx.set_damage_score(mode, 0.0)
    ctx.set_quality_rescale(mode)
    ctx.set_damage_profile(mode)
    ctx.set_coverage(mode)
    ctx.set_pileup(mode, *FILTER)
    ctx.set_allele_likelihoods(mode, *FILTER)
    ctx.set_genotype_likelihoods(True)
    ctx.set_snp_panel(mode, *pn.args(p), *FILTER)


def start_over(ctx, p, mode):
    """a context that has counted batches, back to the nine stages in `mode` with nothing counted (a stage set to the mode it has keeps what it holds: reset by name)"""
    all_stages(ctx, p, mode)
    for reset in (ctx.duplicates_reset, ctx.reset_damage_scores, ctx.reset_quality_rescale, ctx.reset_damage_profile, ctx.reset_coverage, ctx.pileup_reset, ctx.allele_reset,
                  ctx.snp_panel_reset):
        reset()


def _plain(x):
    """a read-out without its time fields, arrays as bytes: equal iff every word is"""
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items() if not k.endswith("_ms") and k not in ("slots", "grows")}  # (the duplicate table's geometry is not its content)
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return x


def snapshot(ctx, p):
    """every table, summary word, call and histogram the nine stages keep in a context"""
    n_rows = len(p["tid"])
    s = {"damage": ctx.damage_profile(), "coverage": ctx.coverage(), "pileup": ctx.pileup(2, 60), "allele": ctx.allele_summary(2, 3.0), "genotype": ctx.genotype_summary(2, 3.0, 1.0),
         "panel": ctx.snp_panel(RULE), "panel_counts": ctx.snp_panel_counts(0, n_rows), "panel_calls": ctx.snp_panel_calls(0, n_rows, RULE),
         "duplicates": ctx.duplicates(), "scores": ctx.damage_scores(), "rescale": ctx.quality_rescale()}
    for tid, n in enumerate(LENGTHS):
        s[f"depth{tid}"] = ctx.coverage_depth(tid, 0, n)
        s[f"pileup{tid}"] = ctx.pileup_counts(tid, 0, n)
        s[f"consensus{tid}"] = ctx.pileup_consensus(tid, 0, n, 2, 60)
        s[f"allele{tid}"] = ctx.allele_cells(tid, 0, n)
        s[f"allele_calls{tid}"] = ctx.allele_consensus(tid, 0, n, 2, 3.0)
        s[f"het{tid}"] = ctx.genotype_cells(tid, 0, n)
        s[f"genotypes{tid}"] = ctx.genotype_calls(tid, 0, n, 2, 3.0, 1.0)
    return _plain(s)


def assert_same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            for kk in a[k]:
                assert a[k][kk] == b[k][kk], (what, k, kk, a[k][kk] if not isinstance(a[k][kk], tuple) else "array")
        assert a[k] == b[k], (what, k)


def mapped_records(idx, params, p, batch, mode):
    """context A: the batch mapped with all nine stages on and converted to records -> (records, rescaled qualities, snapshot, the fetched result's hits and ops)"""
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        all_stages(ctx, p, mode)
        res = ctx.map_batch(*batch)
        recs, rescaled = ctx.hits_to_records(res, *batch, seed=SEED, rescaled=True)
        tracks = [_reported(res, i, r) for i, r in enumerate(recs)]
        return recs, rescaled, snapshot(ctx, p), tracks
    finally:
        ctx.close()


def _reported(res, i, rec):
    """the sorted operations of the hit a record reports: of the read's hits with the record's AS whose track has its CIGAR's length (nearly always one)"""
    if not rec["mapped"]:
        return None
    want = sum(n for n, op in au.cigar_ops(rec["cigar"]))
    found = [np.sort(h["ops_raw"]) for h in res.hits(i) if h["score"] == rec["as"] and len(h["ops_raw"]) == want]
    assert found, ("no hit matches the record", i, rec)
    return found


def test_device_tracks_equal_host_tracks(world):
    _, idx, _ = world
    rng = np.random.default_rng(8)
    table = au.shapes(LENGTHS)
    pairs = [(t[1], t[2]) for t in table] + au.random_alignments(rng, 3000, LENGTHS)
    order = rng.permutation(len(pairs))
    recs, lens = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    offsets = au.offsets_of(lens)
    seqs = rng.choice(np.frombuffer(b"ACGTN", np.uint8), int(offsets[-1]))
    quals = rng.integers(0, 42, int(offsets[-1])).astype(np.uint8)
    arrays = mapad_amd.pack_alignments(recs)
    for model in MODELS:
        params = mapad_amd.make_params(resolve_params(MODELS[model]))
        host = mapad_amd.alignment_tracks_host(idx, params, offsets, *arrays, min_mapq=10)
        au.assert_tracks(host, recs, lens, LENGTHS, min_mapq=10, start_at_end=model == "ss")
        ctx = mapad_amd.Context(idx, params, 0)
        try:
            out = ctx.accumulate_alignments(seqs, quals, offsets, *arrays, min_mapq=10)  # (no stage is on: the tracks alone)
            dev = ctx.alignment_tracks()
            au.same_tracks(host, dev)
            assert np.array_equal(out["status_class"], host["status_class"]) and out["class_counts"] == host["class_counts"] and out["build_ms"] > 0.0
            assert all(out["class_counts"][k] >= 1 for k in au.CLASSES)
            assert out["duplicate"] is None and out["scored"] is None and out["rescaled"] is None
            with pytest.raises(mapad_amd.MapadError):  # a batch of alignments has no search result
                ctx.fetch()
        finally:
            ctx.close()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("model", list(MODELS))
def test_round_trip_equals_the_context_that_mapped(world, model, mode):
    g, idx, p = world
    params = mapad_amd.make_params(resolve_params(MODELS[model]))
    batch = du.with_duplicates(pn.mixed_batch(g, 2500, seed=5), 800, seed=3)
    n = len(batch[2]) - 1
    recs, rescaled, want, tracks = mapped_records(idx, params, p, batch, mode)
    # the batch exercises the hard shapes: equality cannot be vacuous
    assert any(not r["mapped"] for r in recs) and any(r["mapped"] and r["reverse"] for r in recs) and any(r["duplicate"] for r in recs)
    assert any(r["mapped"] and b"N" in batch[0][int(batch[2][i]):int(batch[2][i + 1])].tobytes() for i, r in enumerate(recs))
    # (TEST_MODEL's threshold admits no gap: deletions and insertions are held against a search for "ss" only.  The position a Deletion carries under a model that
    # starts in the middle of the read — align_op_word's q - 1 / q around L / 2 — is therefore NOT verified against a search here, only against the rule written
    # again in analyse_util.expected_track; no stage reads that field.)
    if model == "ss":
        assert any(r["mapped"] and r["reverse"] and "D" in r["cigar"] for r in recs) and any(r["mapped"] and "I" in r["cigar"] for r in recs)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        all_stages(ctx, p, mode)
        out = ctx.accumulate_alignments(*batch, *au.alignments_of(recs))
        got = snapshot(ctx, p)
        dev = ctx.alignment_tracks()
    finally:
        ctx.close()
    assert_same(want, got, f"{model}, mode {mode}")
    assert want["coverage"]["reads"] > 0 and want["panel"]["reads_on_panel"] > 0 and want["scores"]["reads_scored"] > 0 and want["rescale"]["bases_changed"] > 0
    mapped = np.array([r["mapped"] for r in recs])
    assert np.array_equal(out["status_class"] == 0, mapped) and np.array_equal(out["status_class"] == 1, ~mapped)
    assert out["class_counts"]["ok"] == int(mapped.sum()) and out["class_counts"]["unmapped"] == n - int(mapped.sum())
    assert np.array_equal(out["duplicate"].astype(bool), np.array([r["duplicate"] for r in recs]))
    scored = np.array([r["damage_score"] is not None for r in recs])
    assert np.array_equal(out["scored"].astype(bool), scored)
    assert np.array_equal(out["score_q"][scored], np.array([round(r["damage_score"] * 256) for r in recs if r["damage_score"] is not None], np.int32))
    assert rescaled is not None and np.array_equal(out["rescaled"], rescaled)
    # each read's device-built operations are the search's operations of its reported hit
    for i, r in enumerate(recs):
        h = dev["hits"][i]
        if r["mapped"]:
            mine = np.sort(dev["ops"][int(h["ops_offset"]):int(h["ops_offset"]) + int(h["n_ops"])])
            assert any(np.array_equal(mine, t) for t in tracks[i]), (i, r, [hex(w) for w in mine[:6]], [hex(w) for w in tracks[i][0][:6]])
        else:
            assert h["n_ops"] == 0


def test_batch_cuts_do_not_matter(world):
    g, idx, p = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = du.with_duplicates(pn.mixed_batch(g, 150, seed=21), 70, seed=4)  # (a call per read in the first cut: kept small)
    n = len(batch[2]) - 1
    recs, _, want, _ = mapped_records(idx, params, p, batch, 2)
    first_wins = np.array([r["duplicate"] for r in recs])
    assert n > 7 * 30 and first_wins.any()
    ctx = mapad_amd.Context(idx, params, 0)  # (one context for the three cuts, every table emptied in between)
    results = {}
    try:
        for cut in (1, 7, 1000):
            start_over(ctx, p, 2)
            dup = []
            for lo in range(0, n, cut):
                ids = np.arange(lo, min(lo + cut, n))
                dup.append(ctx.accumulate_alignments(*du.take(batch, ids), *au.alignments_of([recs[i] for i in ids]))["duplicate"])
            results[cut] = (dup, snapshot(ctx, p))
    finally:
        ctx.close()
    for cut, (dup, got) in results.items():
        batches = (n + cut - 1) // cut
        assert np.array_equal(np.concatenate(dup).astype(bool), first_wins), cut  # the first in input order is the original
        for k in want:  # the tables, whatever the cuts; what counts batches says how many there were
            a, b = want[k], got[k]
            if isinstance(a, dict):
                assert b["batches"] == batches and {**a, "batches": 0} == {**b, "batches": 0}, (cut, k)
            else:
                assert a == b, (cut, k)


def test_other_classes_are_seen_not_counted_and_min_mapq_leaves_reads_out(world):
    g, idx, p = world
    params = mapad_amd.make_params(resolve_params(DAMAGE))
    batch = pn.mixed_batch(g, 700, seed=33)
    n = len(batch[2]) - 1
    recs, _, _, _ = mapped_records(idx, params, p, batch, 1)
    ctx = mapad_amd.Context(idx, params, 0)
    try:
        all_stages(ctx, p, 1)
        ctx.accumulate_alignments(*batch, *au.alignments_of(recs))
        before = snapshot(ctx, p)
        # one read of each class but ok: every table stays where it was, each class counts once, reads_seen grows
        bad = [(name, rec, L) for name, rec, L in au.shapes(LENGTHS) if name in ("unmapped", "below_min_mapq", "no_md", "bad_contig", "unsupported_cigar S", "length_mismatch",
                                                                              "md_mismatch short", "off_contig")]
        lens = [t[2] for t in bad]
        offsets = au.offsets_of(lens)
        seqs, quals = np.full(int(offsets[-1]), ord("A"), np.uint8), np.full(int(offsets[-1]), 35, np.uint8)
        out = ctx.accumulate_alignments(seqs, quals, offsets, *mapad_amd.pack_alignments([t[1] for t in bad]), min_mapq=10)
        assert out["class_counts"] == {k: int(k != "ok") for k in au.CLASSES} and sorted(out["status_class"]) == list(range(1, 9))
        after = snapshot(ctx, p)
        for k in before:
            a, b = before[k], after[k]
            if not isinstance(a, dict):
                assert a == b, k
                continue
            assert b["batches"] == 2, k
            seen = {kk for kk in a if kk.startswith("reads_seen")}
            assert all(b[kk] == a[kk] + len(bad) for kk in seen), (k, seen)
            assert {kk: v for kk, v in a.items() if kk not in seen | {"batches"}} == {kk: v for kk, v in b.items() if kk not in seen | {"batches"}}, k
        # MAPQ 0..37 over the records, threshold 30: the tables of an accumulation of only the reads at or above it (reads_seen apart: those reads are seen);
        # the same context, every table emptied first
        mapq = np.random.default_rng(6).integers(0, 38, n)
        keep = np.flatnonzero(mapq >= 30)
        got = {}
        for what in ("threshold", "subset"):
            start_over(ctx, p, 1)
            if what == "threshold":
                out = ctx.accumulate_alignments(*batch, *au.alignments_of(recs, mapq=mapq), min_mapq=30)
                assert out["class_counts"]["below_min_mapq"] == sum(1 for i in range(n) if recs[i]["mapped"] and mapq[i] < 30) > 0
            else:
                ctx.accumulate_alignments(*du.take(batch, keep), *au.alignments_of([recs[i] for i in keep], mapq=mapq[keep]), min_mapq=30)
            got[what] = snapshot(ctx, p)
    finally:
        ctx.close()
    for k in got["threshold"]:
        a, b = got["threshold"][k], got["subset"][k]
        if isinstance(a, dict):
            seen = {kk for kk in a if kk.startswith("reads_seen")}
            assert {kk: v for kk, v in a.items() if kk not in seen} == {kk: v for kk, v in b.items() if kk not in seen}, k
        else:
            assert a == b, k


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
GUARD = ["timeout", "-k", "10", "600"]  # every GPU child process under a time limit of its own
MODEL_FLAGS = ["-l", "single_stranded", "-f", "0.5", "-t", "0.5", "-d", "0.02", "-s", "1.0", "-i", "0.001", "-p", "0.03"]


def _write_fasta(path, contigs):
    with open(path, "w") as f:
        for name, s in contigs:
            f.write(f">{name}\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60].tobytes().decode() + "\n")


def test_cli_analyse_of_the_bam_map_wrote_gives_maps_reports_and_records(tmp_path):
    """`mapad-amd map` with every report option, then `mapad-amd analyse` of its BAM with the same options: every report file byte for byte (none holds a time),
    and -o the same records — flags, QUAL, OQ, DS and every other tag"""
    import subprocess

    from mapad_amd import build as mbuild
    from mapad_amd import synth

    import pileup_util as pu
    from bam_util import read_bam
    mapad_amd.lib()
    cli = mbuild.build_cli()
    g = synth.genome(120_000, seed=17)
    g[90_000:90_300] = g[30_000:30_300]
    split = 70_003
    fa, fq, snp = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fastq"), str(tmp_path / "panel.snp")
    _write_fasta(fa, [("chr1", g[:split]), ("X", g[split:])])
    u = synth.reads(g, 2500, seed=23, qual_range=(20, 40), damage=pn.DMG, len_range=(25, 110), indel_frac=0.3)
    rep = synth.reads(g[30_000:30_300], 200, 40, seed=24, qual_range=(20, 40), exo_frac=0.0)
    seqs, quals, offsets = du.with_duplicates(pu.concat(u, rep, pu.hand_made([g[0:40], g[split - 40:split], g[120_000 - 40:120_000]], qual=31)), 900, seed=13)
    with open(fq, "w") as f:
        for i in range(len(offsets) - 1):
            s, e = int(offsets[i]), int(offsets[i + 1])
            f.write(f"@r{i}\n{seqs[s:e].tobytes().decode()}\n+\n{''.join(chr(33 + q) for q in quals[s:e])}\n")
    xs = sorted(set(range(0, 120_000, 37)) | {0, split - 1, split, 120_000 - 1})
    with open(snp, "w") as f:
        for i, x in enumerate(xs):
            f.write(f"rs{i}\t{'1' if x < split else '23'}\t0.0\t{x - (split if x >= split else 0) + 1}\t{chr(g[x])}\t{chr(pn._next(g[x], 1 + (i & 1)))}\n")
    subprocess.check_call(GUARD + [cli, "index", "-g", fa])
    files = ("damage", "coverage", "pileup", "consensus", "allele", "dcons", "dcons_qual", "vcf", "gt_tsv", "duplicates", "ds_hist", "rescale", "geno", "psnp", "ind", "counts",
             "panel_report")

    def options(tag):
        o = {k: str(tmp_path / f"{tag}.{k}") for k in files + ("bam",)}
        return o, ["--damage_profile", o["damage"], "--coverage", o["coverage"], "--pileup", o["pileup"], "--pileup_min_bq", "25", "--pileup_mask5", "2", "--consensus", o["consensus"],
                   "--consensus_min_depth", "2", "--allele_likelihoods", o["allele"], "--allele_min_bq", "20", "--damage_consensus", o["dcons"], "--damage_consensus_qual",
                   o["dcons_qual"], "--genotype_vcf", o["vcf"], "--genotype_likelihoods", o["gt_tsv"], "--mark_duplicates", "--duplicates", o["duplicates"], "--damage_score",
                   "--damage_score_hist", o["ds_hist"], "--rescale_qualities", "--rescale_pileup", "--rescale_keep_original", "--rescale_report", o["rescale"], "--snp_panel", snp,
                   "--panel_geno", o["geno"], "--panel_snp", o["psnp"], "--panel_ind", o["ind"], "--panel_counts", o["counts"], "--panel_report", o["panel_report"],
                   "--panel_min_bq", "30", "--panel_transitions", "single_strand", "--panel_seed", "9", "-o", o["bam"]]

    a, a_opts = options("a")
    subprocess.check_call(GUARD + [cli, "map", "-r", fq, "-g", fa, "--seed", "7"] + MODEL_FLAGS + a_opts)
    b, b_opts = options("b")
    report = str(tmp_path / "b.analyse")
    # (--original_qualities: the stages see OQ where map kept it, so that the rescaling starts from the bytes map started from)
    pr = subprocess.run(GUARD + [cli, "analyse", "--reads", a["bam"], "-g", fa, "--analyse_report", report, "--original_qualities"] + MODEL_FLAGS + b_opts, check=True,
                        stderr=subprocess.PIPE, text=True)
    assert "analyse:" in pr.stderr and "track build" in pr.stderr, pr.stderr
    for k in files:
        assert open(a[k], "rb").read() == open(b[k], "rb").read(), k
    ta, _, ra = read_bam(a["bam"])
    tb, _, rb = read_bam(b["bam"])
    assert len(ra) == len(offsets) - 1 and ra == rb
    assert any(r["flags"] & 0x400 for r in ra) and any("OQ" in r["tags"] for r in ra) and any("DS" in r["tags"] for r in ra) and any(r["flags"] & 0x4 for r in ra)
    assert tb.startswith(ta) and tb[len(ta):].startswith("@PG\tID:mapAD.analyse\t") and tb.count("\n") == ta.count("\n") + 1
    rep = dict(ln.split("\t") for ln in open(report).read().splitlines()[1:])
    mapped = sum(1 for r in ra if not r["flags"] & 0x4)
    assert int(rep["records"]) == len(ra) and int(rep["ok"]) == mapped and int(rep["unmapped"]) == len(ra) - mapped and int(rep["batches"]) == 1
    assert int(rep["records_written"]) == len(ra) and float(rep["track_build_reads_per_s"]) > 0
    # --exclude_duplicates drops exactly the records map flagged, in input order, and touches nothing else of the others
    c = str(tmp_path / "c.bam")
    subprocess.check_call(GUARD + [cli, "analyse", "--reads", a["bam"], "-g", fa, "--exclude_duplicates", "-o", c])
    assert read_bam(c)[2] == [r for r in ra if not r["flags"] & 0x400]
    # a threshold on MAPQ counts fewer reads
    subprocess.check_call(GUARD + [cli, "analyse", "--reads", a["bam"], "-g", fa, "--min_mapq", "30", "--coverage", str(tmp_path / "c.cov")])
    head = open(str(tmp_path / "c.cov")).readline()
    assert int(head.split("reads=")[1].split()[0]) < int(open(a["coverage"]).readline().split("reads=")[1].split()[0])


def test_cli_analyse_reports_the_records_it_cannot_count(tmp_path):
    """a hand-made BAM: a soft-clipped record and a record without MD are counted in their classes, not fatal; a BAM whose mapped records all lack MD is an error"""
    import subprocess

    from mapad_amd import build as mbuild
    from mapad_amd import synth
    mapad_amd.lib()
    cli = mbuild.build_cli()
    g = synth.genome(6_000, seed=3)
    fa = str(tmp_path / "ref.fa")
    _write_fasta(fa, [("c1", g[:4_000]), ("c2", g[4_000:])])
    subprocess.check_call(GUARD + [cli, "index", "-g", fa])
    refs = [("c1", 4_000), ("c2", 2_000)]
    piece = lambda lo, hi: g[lo:hi].tobytes().decode()  # noqa: E731
    deleted = piece(4_100, 4_120) + piece(4_122, 4_140)  # c2:100, two bases deleted behind the 20th
    recs = [{"name": "ok", "flags": 0, "tid": 0, "pos": 100, "mapq": 37, "cigar": "30M", "seq": piece(100, 130), "qual": "I" * 30, "tags": [("MD", "Z", "30"), ("X0", "i", 1)]},
            {"name": "clipped", "flags": 0, "tid": 0, "pos": 205, "mapq": 37, "cigar": "5S25M", "seq": piece(200, 230), "qual": "I" * 30, "tags": [("MD", "Z", "25")]},
            {"name": "no_md", "flags": 0, "tid": 0, "pos": 300, "mapq": 37, "cigar": "30M", "seq": piece(300, 330), "qual": "I" * 30, "tags": [("NM", "i", 0)]},
            {"name": "unmapped", "flags": 4, "seq": piece(400, 430), "qual": "I" * 30, "tags": []},
            {"name": "deletion", "flags": 16, "tid": 1, "pos": 100, "mapq": 20, "cigar": "20M2D18M", "seq": deleted, "qual": "I" * 38,
             "tags": [("MD", "Z", "20^" + piece(4_120, 4_122) + "18")]}]
    bam, cov, report = str(tmp_path / "in.bam"), str(tmp_path / "cov.tsv"), str(tmp_path / "report.tsv")
    au.write_aligned_bam(bam, "@HD\tVN:1.6\n", refs, recs)
    subprocess.check_call(GUARD + [cli, "analyse", "--reads", bam, "-g", fa, "--coverage", cov, "--analyse_report", report] + MODEL_FLAGS)
    rep = dict(ln.split("\t") for ln in open(report).read().splitlines()[1:])
    want = {"records": 5, "ok": 2, "unmapped": 1, "below_min_mapq": 0, "no_md": 1, "bad_contig": 0, "unsupported_cigar": 1, "length_mismatch": 0, "md_mismatch": 0, "off_contig": 0,
            "batches": 1}
    assert {k: int(rep[k]) for k in want} == want
    lines = open(cov).read().splitlines()
    assert "reads=2 reads_seen=5" in lines[0]
    rows = {ln.split("\t")[0]: ln.split("\t") for ln in lines[2:4]}
    assert (rows["c1"][3], rows["c1"][4], rows["c2"][3], rows["c2"][4]) == ("1", "30", "1", "38")  # the deleted bases are not covered
    # with --min_mapq 30 the reverse record leaves
    subprocess.check_call(GUARD + [cli, "analyse", "--reads", bam, "-g", fa, "--coverage", cov, "--analyse_report", report, "--min_mapq", "30"] + MODEL_FLAGS)
    rep = dict(ln.split("\t") for ln in open(report).read().splitlines()[1:])
    assert (int(rep["ok"]), int(rep["below_min_mapq"])) == (1, 1)
    # every mapped record without MD: an error that says so
    for r in recs:
        r["tags"] = [t for t in r["tags"] if t[0] != "MD"]
    au.write_aligned_bam(bam, "@HD\tVN:1.6\n", refs, recs)
    pr = subprocess.run(GUARD + [cli, "analyse", "--reads", bam, "-g", fa, "--coverage", cov] + MODEL_FLAGS, stderr=subprocess.PIPE, text=True)
    assert pr.returncode != 0 and "MD:Z" in pr.stderr, pr.stderr
    # a BAM whose reference list is not the index's contigs (another order, another length) is refused, not counted under the wrong contigs
    for other in ([("c2", 2_000), ("c1", 4_000)], [("c1", 4_000), ("c2", 1_999)], [("c1", 4_000)]):
        au.write_aligned_bam(bam, "@HD\tVN:1.6\n", other, recs)
        pr = subprocess.run(GUARD + [cli, "analyse", "--reads", bam, "-g", fa, "--coverage", cov], stderr=subprocess.PIPE, text=True)
        assert pr.returncode != 0 and "reference sequence" in pr.stderr, pr.stderr
    # the stages that score with the damage model ask for it, as map does
    pr = subprocess.run(GUARD + [cli, "analyse", "--reads", bam, "-g", fa, "--damage_score"], stderr=subprocess.PIPE, text=True)
    assert pr.returncode != 0 and "is required" in pr.stderr, pr.stderr
