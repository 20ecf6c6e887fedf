"""Case table of the search parity over the whole base-quality byte and the whole read alphabet (tests/test_gpu_quality.py on the GPU, tests/test_quality_host.py
through the host build of the kernels' per-read logic): one table, two runners, like tests/sweep_util.py.

The reference does not clamp the quality byte (sequence_difference_models.rs:9: MAX_ENCODED_BASE_QUALITY = u8::MAX; :287-293: the model caches all 256 levels) and
the product builds score tables of 256 quality rows to match (host_models.hpp: add_length, quality_levels); every other search test draws qualities from 20-40.
Collapsed read pairs carry Q41-Q93, BAM records without qualities 0xFF at every position, Illumina writes Q2 and Q0 under N.  At Q0 and Q1 the model's optimal
symbol is a MISMATCH (simple_adna_get: no_err = 1 - 3e < e): sdm_optimal is not the match value, a match costs a penalty, and the D array gains nothing there.
The read alphabet: exactly `ACGT` have a class, every other byte is class 4 (common.hpp: base_index; the reference's get_min_penalty:
!DNA_UPPERCASE_ALPHABET.contains(&to)).

World: sweep_util.grid_world().  Reads: sweep_util.grid_reads (35-70 bp, damaged, a tenth with indels) with their qualities or symbols rewritten by a seeded generator.
Every case carries a reach-condition on the ORACLE's result (conditions, not measurements: the floors are about half of what the oracle yields)."""
import numpy as np

from kat_util import resolve_params
from parity_util import CONTINUOUS, DAMAGE, DOUBLE_STRANDED, IGNORE_BQ, NO_DAMAGE, VINDIJA, split_reads
from sweep_util import GRID_MAX_POPS, gapped_hits, hits_per_read, pack

OP_MISMATCH, OP_MATCH = 3, 2  # common.hpp: the kind in the top byte of a packed edit operation, the read position in the low 16 bits

PRESETS = {"damage": DAMAGE, "no_damage": NO_DAMAGE, "continuous": CONTINUOUS, "double_stranded": DOUBLE_STRANDED, "vindija": VINDIJA, "ignore_bq": IGNORE_BQ}
FOUR = ("damage", "no_damage", "continuous", "double_stranded")
QUALITY_BLIND = ("vindija", "ignore_bq")  # one quality level in the model: the quality bytes must make no difference

# every byte the `symbols` case writes into a read: lower case, the ambiguity codes, U, what alignment files use for gaps and padding, and the ends of the byte
SYMBOLS = [ord(c) for c in "acgtnRYKMSWBDHVU.-*"] + [0x00, 0xFF]


def _low(rng, n):
    return rng.integers(0, 2, n).astype(np.uint8)  # Q0 or Q1


def _one_low(reads, qs, rng):
    for q in qs:
        q[int(rng.integers(0, len(q)))] = _low(rng, 1)[0]


def _ends_low(reads, qs, rng):
    for i, q in enumerate(qs):  # first base, last base, first, last, ...; Q0, Q0, Q1, Q1, ...
        q[0 if i % 2 == 0 else -1] = (i // 2) % 2


def _two_low(reads, qs, rng):
    for q in qs:
        q[rng.choice(len(q), 2, replace=False)] = _low(rng, 2)


def _n_low(reads, qs, rng):
    for r, q in zip(reads, qs):  # one N, or two; at Q0 or Q2 (what Illumina writes under an N)
        at = rng.choice(len(q), 1 + int(rng.integers(0, 2)), replace=False)
        r[at] = ord("N")
        q[at] = 2 * rng.integers(0, 2, len(at))


def _symbols(reads, qs, rng):
    for i, r in enumerate(reads):
        r[int(rng.integers(0, len(r)))] = SYMBOLS[i % len(SYMBOLS)]


def _q41_93(reads, qs, rng):
    for q in qs:
        q[:] = rng.integers(41, 94, len(q))


def _q255(reads, qs, rng):
    for q in qs:
        q[:] = 255


def _full_byte(reads, qs, rng):
    for q in qs:
        q[:] = rng.integers(0, 256, len(q))


def _ladder(reads, qs, rng):
    n = len(qs)
    for i, q in enumerate(qs):  # the read's quality centre climbs from 0 to 255 over the batch; every base within 3 of it
        q[:] = np.clip(i * 255 // (n - 1) + rng.integers(-3, 4, len(q)), 0, 255)


# id -> (rewrite, seed, the presets it runs under, reach: floors on the oracle's result)
#   mm_low / match_low: hits whose edit track has OP_MISMATCH / OP_MATCH on a base of quality < 2;  mm_n: hits with a mismatch on an N;  gapped: hits with an indel
CASES = {
    "one_low": (_one_low, 1, FOUR, dict(mm_low=5, match_low=50)),
    "ends_low": (_ends_low, 2, FOUR, dict(mm_low=20, match_low=50)),
    # (not under CONTINUOUS: the oracle's longest search of that cell takes 134 112 pops, past 2^17; every second read of it would stay inside and map 36 reads)
    "two_low": (_two_low, 3, ("damage", "no_damage", "double_stranded"), dict(mm_low=5, match_low=50)),
    "n_low": (_n_low, 4, FOUR + QUALITY_BLIND, dict(mm_n=50, gapped=5)),
    "symbols": (_symbols, 5, FOUR + QUALITY_BLIND, dict(every_symbol=True)),
    "q41_93": (_q41_93, 6, FOUR, {}),
    "q255": (_q255, 7, FOUR, {}),
    "full_byte": (_full_byte, 8, FOUR, {}),
}
CELLS = [(cid, preset) for cid, (_, _, presets, _) in CASES.items() for preset in presets]
CELL_IDS = [f"{cid}-{preset}" for cid, preset in CELLS]
# the launch variants (GPU only): (case id, preset, environment)
LAUNCH_VARIANTS = ([(cid, "damage", env) for cid in ("one_low", "ends_low", "full_byte")
                    for env in ({"MAPAD_LANES_PER_READ": "2"}, {"MAPAD_LANES_PER_READ": "1"}, {"MAPAD_GENERAL_DIRECTION": "1"})]
                   + [("full_byte", "damage", {"MAPAD_NEAR_LDS": "0"})])
LADDER_SEED = 9
MIN_MAPPED = 50


def params(preset):
    return resolve_params(PRESETS[preset])


def rewritten(world, rewrite, seed):
    """grid_reads with their qualities or symbols rewritten -> a batch of its own (the world's batch stays as it is)"""
    reads, qs = split_reads(*world.grid_batch)
    reads = [np.frombuffer(r, np.uint8).copy() for r in reads]
    qs = [q.copy() for q in qs]
    rewrite(reads, qs, np.random.default_rng(seed))
    return pack(reads, qs)


def _cached(world, key, rewrite, seed):
    """the rewritten batch `key` of a world, made once"""
    cache = world.__dict__.setdefault("_quality_batches", {})
    if key not in cache:
        cache[key] = rewritten(world, rewrite, seed)
    return cache[key]


def case_batch(world, cid):
    return _cached(world, cid, *CASES[cid][:2])


def q40_batch(batch):
    """the same reads with every quality at 40"""
    return batch[0], np.full_like(batch[1], 40), batch[2]


def ladder_batch(world):
    return _cached(world, "ladder", _ladder, LADDER_SEED)


def oracle(world, cid, preset):
    return world.oracle(("quality", cid, preset), params(preset), case_batch(world, cid))


def ladder_oracle(world):
    return world.oracle(("quality", "ladder"), params("damage"), ladder_batch(world))


def subset(batch, sel):
    reads, qs = split_reads(*batch)
    return pack([np.frombuffer(reads[i], np.uint8) for i in sel], [qs[i] for i in sel])


# ---- reach ----------------------------------------------------------------------------------------------------------------------------------------------------
def _ops_by_hit(ores, batch):
    """per edit operation of the oracle's result: (its hit, its kind, the read's symbol and quality at its read position)"""
    seqs, quals, offsets = batch
    n_ops = np.diff(ores.op_offsets.astype(np.int64))
    hit = np.repeat(np.arange(len(n_ops)), n_ops)
    read_of_hit = np.repeat(np.arange(ores.n), hits_per_read(ores))
    at = offsets.astype(np.int64)[read_of_hit[hit]] + (ores.ops & 0xFFFF).astype(np.int64)
    return hit, (ores.ops >> 24).astype(np.uint8), seqs[at], quals[at]


def reach_counts(ores, batch):
    hit, kind, sym, q = _ops_by_hit(ores, batch)
    low = q < 2
    mapped = hits_per_read(ores) > 0
    seqs, _, offsets = batch
    in_mapped = np.repeat(mapped, np.diff(offsets.astype(np.int64)))
    return dict(mapped=int(mapped.sum()), max_pops=int(ores.counters[:, 3].max()),
                mm_low=len(np.unique(hit[(kind == OP_MISMATCH) & low])), match_low=len(np.unique(hit[(kind == OP_MATCH) & low])),
                mm_n=len(np.unique(hit[(kind == OP_MISMATCH) & (sym == ord("N"))])), match_n=len(np.unique(hit[(kind == OP_MATCH) & (sym == ord("N"))])),
                gapped=int(gapped_hits(ores).sum()), symbols_in_mapped_reads=sorted(set(SYMBOLS) & set(np.unique(seqs[in_mapped]).tolist())))


def check_reach(cid, preset, ores, batch):
    """-> the counts (the runners print them)"""
    c = reach_counts(ores, batch)
    floors = CASES[cid][3]
    assert c["mapped"] >= MIN_MAPPED, (cid, preset, c)
    assert c["max_pops"] < GRID_MAX_POPS, (cid, preset, c)  # the GPU search answers, not the host tail
    for k in ("mm_low", "match_low", "mm_n", "gapped"):
        assert c[k] >= floors.get(k, 0), (cid, preset, k, c)
    if floors.get("every_symbol"):
        assert c["symbols_in_mapped_reads"] == sorted(SYMBOLS), (cid, preset, c)
    assert c["match_n"] == 0  # a Match is only ever emitted for a read base that is one of ACGT
    return c


def same_oracle_results(a, b):
    """two oracle results word for word: hits, heap order, score bits, edit tracks, D arrays, counters"""
    assert a.n == b.n and np.array_equal(a.hit_offsets, b.hit_offsets) and np.array_equal(a.intervals, b.intervals)
    assert np.array_equal(a.scores.view(np.uint32), b.scores.view(np.uint32)) and np.array_equal(a.op_offsets, b.op_offsets) and np.array_equal(a.ops, b.ops)
    assert np.array_equal(a.counters, b.counters)
    for i in range(a.n):
        assert np.array_equal(a.d_array(i).view(np.uint32), b.d_array(i).view(np.uint32)), i


def check_quality_blind(world, cid, preset):
    """VINDIJA and IGNORE_BQ: the oracle's result of the case equals its result of the same reads at quality 40"""
    batch = case_batch(world, cid)
    assert (batch[1] != 40).any()
    same_oracle_results(oracle(world, cid, preset), world.oracle(("quality", cid, preset, "q40"), params(preset), q40_batch(batch)))


# ---- records --------------------------------------------------------------------------------------------------------------------------------------------------
RECORD_CASES = ("one_low", "ends_low", "n_low", "symbols", "q255", "full_byte")  # each under records_util.PRESETS: damage and no_damage


def record_world(world):
    """records_util's wiring (the product's suffix-array samples under the oracle's own LF walk, the contig table) over the grid world's index"""
    import records_util as ru
    return ru.RecordWorld.from_index(world.pidx, world.contigs, 32)


def check_record_reach(cid, genome, recs, text, batch):
    """Ground truth that needs no index: NM of every ungapped record is the number of positions at which the read differs from the text it was laid on — a read byte
    outside ACGT differs from every reference base (parity_util.check_ungapped_records_against_the_text).  -> the counts"""
    from parity_util import check_ungapped_records_against_the_text
    m = recs["mapped"] != 0
    checked, failed = check_ungapped_records_against_the_text(genome, recs, text, batch[0], batch[2])
    c = dict(mapped=int(m.sum()), ungapped_checked=checked, mapq_values=len(np.unique(recs["mapq"][m])), nm_0=int((recs["nm"][m] == 0).sum()))
    assert c["mapped"] >= MIN_MAPPED and checked >= MIN_MAPPED and failed == 0, (cid, c, failed)
    if cid in ("n_low", "symbols"):  # every read of these cases holds a byte outside ACGT
        assert c["nm_0"] == 0, (cid, c)
    return c


# ---- accumulators at the ends of the quality axis ---------------------------------------------------------------------------------------------------------------
def _edges(reads, qs, rng):
    for i, q in enumerate(qs):  # qualities in {0, 1, 254, 255}: one base at Q0 or Q1 (whole reads of them would take millions of pops), every other at 254 or 255
        q[:] = rng.integers(254, 256, len(q))
        q[int(rng.integers(0, len(q)))] = i % 2


ACC_BATCHES = ("full_byte", "q255", "edges")
EDGES_SEED = 10  # of the generator that writes the `edges` batch
ACC_SEED = 99    # of the records (the stand-ins for rand::rng())
ACC_ALLELE_RULE, ACC_GENOTYPE_RULE, ACC_PILEUP_RULE = (1, 3.0), (1, 3.0, 0.0), (1, 0)
ACC_MIN_BQ = (0, 1, 255)  # the library refuses 256 (mapad_ctx_set_pileup: MAPAD_ERR_INVALID)


def acc_batch(world, name):
    return _cached(world, "edges", _edges, EDGES_SEED) if name == "edges" else case_batch(world, name)


def m_column_qualities(recs, batch):
    """the qualities of the bases A, C, G, T of the mapped reads that stand in an M column: what a pileup without masks can count"""
    import re
    from pileup_util import record_rows
    is_acgt = np.isin(np.arange(256), np.frombuffer(b"ACGT", np.uint8))  # exactly these four, as common.hpp: base_index has it (no case folding)
    out = []
    for mapped, _, _, cigar, seq, qual, _, _ in record_rows(recs, *batch):
        i = 0
        for n, op in re.findall(r"(\d+)([MID])", cigar) if mapped else ():
            n = int(n)
            if op == "M":
                out.append(qual[i:i + n][is_acgt[seq[i:i + n]]])
            i += n if op != "D" else 0
    return np.concatenate(out).astype(np.int64)


def check_accumulator_reach(name, quals_counted):
    q = quals_counted
    assert len(q) > 2000, (name, len(q))
    if name == "q255":
        assert (q == 255).all()
    elif name == "edges":
        assert set(np.unique(q).tolist()) == {0, 1, 254, 255} and min((q == 0).sum(), (q == 1).sum()) >= 20, (name, np.bincount(q, minlength=256)[[0, 1, 254, 255]])
    else:
        assert len(np.unique(q)) == 256 and (q == 0).sum() >= 10 and (q == 255).sum() >= 10, (name, len(np.unique(q)))


def check_low_quality_moves(name, by_min_bq, quals_counted):
    """by_min_bq: {min_bq: a pileup summary}: columns_low_quality is exactly the bases below the threshold, and they are what columns_counted loses"""
    for min_bq, s in by_min_bq.items():
        below = int((quals_counted < min_bq).sum())
        assert s["columns_low_quality"] == below and s["columns_counted"] == len(quals_counted) - below, (name, min_bq, s["columns_low_quality"], s["columns_counted"], below)
        assert s["columns_masked"] == 0
    assert by_min_bq[0]["columns_low_quality"] == 0
    if name != "q255":
        assert 0 < by_min_bq[1]["columns_low_quality"] < by_min_bq[255]["columns_low_quality"], name


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------------
CLI_PRESET = "damage"
CLI_SEED = 0


def cli_world(fa, run):
    """the grid genome as FASTA at `fa`, indexed by `mapad-amd index`, opened again -> records_util's wiring over that index"""
    import cli_audit_util as au
    import mapad_amd
    import records_util as ru
    from mapad_amd import synth
    from sweep_util import GRID_GENOME
    contigs = [("chr1", synth.genome(**GRID_GENOME))]
    au.write_fasta(fa, contigs)
    run([au.cli(), "--seed", str(au.INDEX_SEED), "index", "-g", fa])
    return ru.RecordWorld.from_index(mapad_amd.Index.open(fa), contigs, au.sa_sampling_rate(fa))


def cli_inputs(genome):
    """-> {"fastq": records whose quality strings use every character from `!` to `~` (Q0-Q93), "bam": records with 0xFF at every position (a BAM record
    without qualities) and records of raw qualities 94-254; every second one flagged 0x10 (stored reversed and complemented)}: cli_audit_util's input records"""
    from sweep_util import grid_reads
    reads, _ = split_reads(*grid_reads(genome))
    rng = np.random.default_rng(11)
    out = {"fastq": [], "bam": []}
    for i, r in enumerate(reads):
        q = rng.integers(0, 94, len(r))
        out["fastq"].append(dict(name=f"fq{i}", seq=r.decode(), qual="".join(chr(33 + int(x)) for x in q), flags=0, tags=[], mappable=True))
        q = np.full(len(r), 255) if i % 3 == 0 else rng.integers(94, 255, len(r))
        out["bam"].append(dict(name=f"bam{i}", seq=r.decode(), qual="".join(chr(33 + int(x)) for x in q), flags=0x10 if i % 2 else 0, tags=[], mappable=True))
    used = set("".join(r["qual"] for r in out["fastq"]))
    assert used == {chr(c) for c in range(ord("!"), ord("~") + 1)}
    raw = np.concatenate([np.array([ord(c) - 33 for c in r["qual"]]) for r in out["bam"]])
    assert set(np.unique(raw).tolist()) == set(range(94, 256))
    return out


def cli_write_inputs(dirname, inputs):
    """-> {"fastq": path, "bam": path}; a record flagged 0x10 is stored reversed and complemented (record.rs:157-160)"""
    import os
    import cli_audit_util as au
    from bam_util import write_bam
    fq, bam = os.path.join(dirname, "in.fastq"), os.path.join(dirname, "in.bam")
    with open(fq, "w") as f:
        f.write("".join(f"@{r['name']}\n{r['seq']}\n+\n{r['qual']}\n" for r in inputs["fastq"]))
    write_bam(bam, au.HEADER, [], [dict(r, seq=au.revcomp(r["seq"]), qual=r["qual"][::-1]) if r["flags"] & 0x10 else r for r in inputs["bam"]])
    return {"fastq": fq, "bam": bam}


def raw_quals(rec):
    return np.array([ord(c) - 33 for c in rec["qual"]], np.uint8)


def cli_expectation(rworld, recs, n_threads=8):
    """The oracle's own search and its own intervals_to_record over the run's reads as one batch -> (rows as cli_audit_util.compare takes them, the oracle's result).
    (OracleResult.records() writes QUAL + 33 into a line of text, which holds no quality above 93; here the fixed fields come from records_from_hits over the oracle's
    own hits, and SEQ / QUAL are laid out by the writer's rule: reversed — SEQ complemented — on the reverse strand, mapping.rs:795-819.)"""
    import cli_audit_util as au
    from oracle import binding as ob
    oparams = ob.make_params(params(CLI_PRESET))
    ores = rworld.oidx.map_batch(oparams, [r["seq"].encode() for r in recs], [raw_quals(r) for r in recs], n_threads=n_threads)
    orecs, otext = rworld.oidx.records_from_hits(oparams, ores.hit_offsets, ores.intervals, ores.scores, ores.op_offsets, ores.ops, ores.seqs, ores.qs, ores.offsets,
                                                 flags=[r["flags"] for r in recs], n_threads=n_threads)
    text, rows = otext.tobytes().decode(), []
    for r, o in zip(recs, orecs):
        row = dict(flags=int(o["flags"]), tid=int(o["tid"]), pos=int(o["pos"]), mapq=int(o["mapq"]), cigar="*", seq=r["seq"], qual=r["qual"])
        if o["mapped"]:
            a, b, c = int(o["text_off"]), int(o["text_off"]) + int(o["cigar_len"]), int(o["text_off"]) + int(o["cigar_len"]) + int(o["md_len"])
            row.update(cigar=text[a:b], as_bits="%08x" % int(o["as_bits"]), nm=int(o["nm"]), md=text[b:c], xa=text[c:c + int(o["xa_len"])] or "*", x0=int(o["x0"]), x1=int(o["x1"]),
                       xs_bits="%08x" % int(o["xs_bits"]) if o["has_xs"] else "*", xt=chr(int(o["xt"])))
            if o["reverse"]:
                row.update(seq=au.revcomp(r["seq"]), qual=r["qual"][::-1])
        else:
            row.update({k: "*" for k in ("as_bits", "nm", "md", "xa", "x0", "x1", "xs_bits", "xt")})
        rows.append(row)
    return rows, ores


def check_cli_reach(rows):
    m = [r for r in rows if r["as_bits"] != "*"]
    rev = sum(bool(r["flags"] & 0x10) for r in m)
    assert len(m) >= MIN_MAPPED and rev >= 20 and len(m) - rev >= 20 and len({r["mapq"] for r in m}) >= 3, (len(m), rev)


def check_ladder_reach(ores, batch):
    """The ladder is the one case that is meant to leave the GPU search: whole reads at Q0-Q5 take millions of pops.  -> (counts, the reads below 2^17 pops)"""
    c = reach_counts(ores, batch)
    pops = ores.counters[:, 3]
    c["reads_past_2^17"] = int((pops >= GRID_MAX_POPS).sum())
    assert c["mapped"] >= MIN_MAPPED and c["reads_past_2^17"] >= 3 and c["mm_low"] >= 20 and c["match_low"] >= 15, c
    return c, np.flatnonzero(pops < GRID_MAX_POPS)
