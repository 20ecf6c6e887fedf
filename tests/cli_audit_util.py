"""World, input files, expectation and comparison of the audit of the BAM that `mapad-amd map` writes (tests/test_gpu_cli_audit.py: the command line on the GPU;
tests/test_cli_audit_host.py: the host path cut into the command line's slices): one table, two runners, like tests/sweep_util.py and tests/records_util.py.

The expectation is the oracle's own search and its own intervals_to_record (OracleIndex.map_batch(...).records(flags)) over ONE batch of the run's mappable reads in
input order: the command line counts a chunk's first read in mappable reads of the run, so however a run is cut into chunks, slices, launches and devices, read k of the
run draws the stand-ins for rand::rng() of read k (seed 0 on the product side).  The text is world A of records_util (repeats: hit intervals of many rows go through
PrRange, and only there a wrong seed shows), indexed by `mapad-amd index` and opened from disk."""
import gzip
import os
import struct
import subprocess

import numpy as np

import mapad_amd
from mapad_amd import build as mbuild
from mapad_amd import binding as mb
from oracle import binding as ob

import records_util as ru
from bam_util import write_bam
from kat_util import resolve_params
from parity_util import split_reads

SEED = 0
INDEX_SEED = 1234
# the command-line flags of the presets (mapad_amd/presets.py)
CLI_PRESETS = {"damage": dict(l="single_stranded", f=0.5, t=0.5, d=0.02, s=1.0, D=0.02, p=0.03, i=0.001, x=1.0),
               "no_damage": dict(l="single_stranded", f=0.0, t=0.0, d=0.0, s=0.0, D=0.02, p=0.03, i=0.001, x=1.0)}
_LONG = dict(l="library", f="five_prime_overhang", t="three_prime_overhang", d="ds_deamination_rate", s="ss_deamination_rate", D="divergence", p="poisson_prob", i="indel_rate",
             x="gap_extension_penalty")
IN_FLAGS = (0, 0x10, 0x4, 0x1 | 0x40 | 0x8, 0x200, 0x400 | 0x10, 0x1 | 0x80 | 0x20 | 0x2, 0x100, 0x800)
MAPPER_TAGS = ("AS", "MD", "NM", "X0", "X1", "XA", "XD", "XE", "XF", "XG", "XM", "XN", "XO", "XS", "XT")  # dropped from the input (mapping.rs:834-848)
NEW_TAG_ORDER = ("AS", "NM", "MD", "XA", "X0", "X1", "XS", "XT", "XD")  # mapping.rs:850-918
HEADER = "@HD\tVN:1.0\n@RG\tID:A12345\tSM:Sample1\n"
N_DUPLICATES = 300
N_DUPLICATES_OF_REPEATS = 200  # drawn from the reads cut from the repeat contig and the tandem repeat (reads_a: parts 3 and 6)
# input positions of the records that cannot be mapped: an empty read, a read beyond MAPAD_MAX_READ_LEN, an empty read right behind it
UNMAPPABLE_AT = {504: "empty_a", 1500: "too_long", 1501: "empty_b"}
BATCH_SIZES = (301, 97, 3 * 97, 5 * 97)  # what the runs cut the input by: no unmappable record may sit on such a boundary
TOO_LONG = 33_000
_COMP = bytes.maketrans(b"ACGTRYKMBVDH", b"TGCAYRMKVBHD")


def cli():
    mapad_amd.lib()
    return mbuild.build_cli()


def cli_flags(preset):
    out = []
    for k, v in CLI_PRESETS[preset].items():
        out += ["-" + k, str(v)]
    return out


def check_cli_flags_are_the_preset(preset):
    """params_from_cli(<the flags the runs pass>) == make_params(resolve_params(preset)), field by field except chunk_size"""
    got = mapad_amd.params_from_cli(**{_LONG[k]: v for k, v in CLI_PRESETS[preset].items()})
    want = mapad_amd.make_params(resolve_params(ru.PRESETS[preset]))
    for name, ctype in mb.Params._fields_:
        if name == "chunk_size":
            continue
        a, b = getattr(got, name), getattr(want, name)
        same = np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32) if isinstance(a, float) else a == b
        assert same, (preset, name, a, b)


# ---- the index on disk ----------------------------------------------------------------------------------------------------------------------------------------
def write_fasta(path, contigs):
    """the contigs as they are: ambiguity codes, lower case and N runs included"""
    with open(path, "wb") as f:
        for name, seq in contigs:
            f.write(b">" + name.encode() + b"\n")
            b = seq.tobytes()
            for i in range(0, len(b), 70):
                f.write(b[i:i + 70] + b"\n")


def sa_sampling_rate(prefix):
    """The sampling rate in <prefix>.tsa: a snappy frame stream (the index writer emits uncompressed chunks) of bincode {version: u8, sample: Vec<u64>, sampling_rate: u64, ...}"""
    raw = open(prefix + ".tsa", "rb").read()
    data, o = bytearray(), 0
    while o < len(raw):
        kind, ln = raw[o], int.from_bytes(raw[o + 1:o + 4], "little")
        if kind == 0x01:
            data += raw[o + 8:o + 4 + ln]  # behind the chunk's CRC
        else:
            assert kind == 0xFF, "a compressed or unknown chunk: not what the index writer emits"
        o += 4 + ln
    n, = struct.unpack_from("<Q", data, 1)
    rate, = struct.unpack_from("<Q", data, 9 + 8 * n)
    return int(rate)


def indexed_world(fa, run=subprocess.check_call):
    """World A's contigs as FASTA at `fa`, indexed by the command line (the real StdRng draws replace the short N run), opened again -> (RecordWorld over that index, clean)"""
    world0, clean = ru.world_a()
    write_fasta(fa, world0.contigs)
    env = {k: v for k, v in os.environ.items() if k != "MAPAD_INDEX_FIXED_REPLACEMENT"}
    run([cli(), "--seed", str(INDEX_SEED), "index", "-g", fa], env=env)
    world = ru.RecordWorld.from_index(mapad_amd.Index.open(fa), world0.contigs, sa_sampling_rate(fa))
    return world, clean


def header_refs(world):
    return [(name, len(s)) for name, s in world.contigs]


# ---- the run's input ------------------------------------------------------------------------------------------------------------------------------------------
def _tags(i):
    """every third input record: tags that survive between the mapper-owned ones that must be replaced; every seventh: an array tag"""
    t = []
    if i % 3 == 0:
        t += [("XI", "Z", "ACGACGT"), ("AS", "i", -3), ("FF", "i", 3 + i), ("MD", "Z", "7A7"), ("RG", "Z", "A12345"), ("NM", "i", 77)]
    if i % 7 == 0:
        t += [("ZB", "B", ("s", [i % 1000, -5, 300]))]
    return t


def audit_input(world, clean):
    """-> the input records in input order: dicts name, seq / qual (Phred + 33) in the read's own orientation, flags, tags, mappable, copy_of (name of the read a
    duplicate is a byte-identical copy of, or None), base (one of the reads of records_util.reads_a)"""
    batch, _ = ru.reads_a(world, clean)
    reads, quals = split_reads(*batch)
    n = len(reads)
    assert n == 2240
    rng = np.random.default_rng(4711)
    repeats = np.concatenate([np.arange(1400, 1700), np.arange(1960, 2000)])  # reads_a: cut from the repeat contig, cut from the tandem repeat
    src = np.concatenate([rng.choice(repeats, N_DUPLICATES_OF_REPEATS, replace=False), rng.choice(n, N_DUPLICATES - N_DUPLICATES_OF_REPEATS, replace=False)])
    keys = np.concatenate([np.arange(n, dtype=np.float64), rng.uniform(0, n, N_DUPLICATES)])  # a copy lands anywhere, before or behind its original
    recs = []
    for k in np.argsort(keys, kind="stable"):
        i = int(k) if k < n else int(src[k - n])
        recs.append(dict(name=f"r{i}" if k < n else f"copy{k - n}_of_r{i}", seq=reads[i].decode(), qual="".join(chr(33 + int(q)) for q in quals[i]),
                         mappable=True, copy_of=None if k < n else f"r{i}", base=bool(k < n)))
    long_seq = np.resize(clean, TOO_LONG).tobytes().decode()
    for at in sorted(UNMAPPABLE_AT):
        assert all(at % b for b in BATCH_SIZES)
        name = UNMAPPABLE_AT[at]
        seq = long_seq if name == "too_long" else ""
        recs.insert(at, dict(name=name, seq=seq, qual="I" * len(seq), mappable=False, copy_of=None, base=False))
    flags = rng.choice(IN_FLAGS, len(recs))
    for i, r in enumerate(recs):
        r["flags"], r["tags"] = int(flags[i]), _tags(i)
    assert [r["name"] for at, r in enumerate(recs) if at in UNMAPPABLE_AT] == [UNMAPPABLE_AT[at] for at in sorted(UNMAPPABLE_AT)]
    return recs


def revcomp(s):
    return s.encode().translate(_COMP)[::-1].decode()


def write_inputs(dirname, recs):
    """the same reads as BAM (flags and tags; a record flagged 0x10 is stored reversed and complemented, record.rs:157-160), FASTQ and FASTQ.gz -> their paths"""
    bam, fq, fqgz = (os.path.join(dirname, "in." + e) for e in ("bam", "fastq", "fastq.gz"))
    write_bam(bam, HEADER, [], [dict(r, seq=revcomp(r["seq"]), qual=r["qual"][::-1]) if r["flags"] & 0x10 else r for r in recs])
    text = "".join(f"@{r['name']}\n{r['seq']}\n+\n{r['qual']}\n" for r in recs)
    with open(fq, "w") as f:
        f.write(text)
    with gzip.open(fqgz, "wt", compresslevel=1) as f:
        f.write(text)
    return {"bam": bam, "fastq": fq, "fastq_gz": fqgz}


def as_fastq(recs):
    """what the FASTQ forms of the input say: no flags, no tags"""
    return [dict(r, flags=0, tags=[]) for r in recs]


def mappable_batch(recs):
    """the run's mappable reads, in input order -> (seqs, quals, offsets)"""
    m = [r for r in recs if r["mappable"]]
    return ob.pack_reads([r["seq"].encode() for r in m], [np.frombuffer(r["qual"].encode(), np.uint8) - 33 for r in m])


def cli_slices(recs, batch_size, n_dev):
    """The slices `--batch_size B` over n_dev devices cuts the run into (main.cpp: a chunk takes B input records; its mappable reads go to the devices in contiguous
    slices, base = n / n_dev with the remainder to the first devices) -> [(first_read, lo, hi)]: reads [first_read + lo, first_read + hi) of the mappable reads"""
    out, first = [], 0
    for c0 in range(0, len(recs), batch_size):
        n = sum(r["mappable"] for r in recs[c0:c0 + batch_size])
        base, extra = divmod(n, n_dev)
        for d in range(n_dev):
            lo = d * base + min(d, extra)
            out.append((first, lo, lo + base + (1 if d < extra else 0)))
        first += n
    return out


# ---- expectation ----------------------------------------------------------------------------------------------------------------------------------------------
def expectation(world, preset, recs, n_threads=8):
    """The oracle's own hits and its own records of the run's mappable reads as one batch -> (rows for the input's flags, rows for an input without flags); a row:
    flags, tid, pos, mapq, cigar, seq, qual in output orientation, as_bits, nm, md, xa, x0, x1, xs_bits, xt ('*' where there is none)"""
    m = [r for r in recs if r["mappable"]]
    ores = world.oidx.map_batch(ob.make_params(resolve_params(ru.PRESETS[preset])), [r["seq"].encode() for r in m],
                                [np.frombuffer(r["qual"].encode(), np.uint8) - 33 for r in m], n_threads=n_threads)
    with_flags, without = ores.records([r["flags"] for r in m]), ores.records([0] * len(m))
    assert len(with_flags) == len(without) == len(m)
    return with_flags, without


def rows_by_input(recs, rows):
    """one entry per input record: its row, None for a record that cannot be mapped"""
    it = iter(rows)
    return [next(it) if r["mappable"] else None for r in recs]


# ---- comparison -----------------------------------------------------------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    """SAM specification 5.3"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def ref_len(cigar):
    n, k = 0, ""
    for ch in cigar:
        if ch.isdigit():
            k += ch
        else:
            n, k = n + (int(k) if ch in "MD" else 0), ""
    return n


def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def differing_fields(got, row, inp, flag_mask=0xFFFF, drop_tags=()):
    """got: a record as bam_util.read_bam gives it (a host-path record adapted by host_record() has neither bin, tag order nor mate fields: those are then not compared);
    row: the oracle's row, None for a record that cannot be mapped; inp: the input record.  -> the names of the fields that differ.  The value of XD is ignored;
    drop_tags: tags of the output that are set aside first."""
    bad = []

    def cmp(name, a, b):
        if a != b:
            bad.append(name)

    tags = {k: v for k, v in got["tags"].items() if k not in drop_tags}
    kept = [t for t in inp["tags"] if t[0] not in MAPPER_TAGS]
    if row is None:
        want = dict(flags=(inp["flags"] & ~(0x8 | 0x20 | 0x2 | 0x100 | 0x800 | 0x10)) | 0x4, tid=-1, pos=-1, cigar="", seq=inp["seq"], qual=inp["qual"])
        mapped = False
    else:
        want = dict(flags=int(row["flags"]), tid=int(row["tid"]), pos=int(row["pos"]), mapq=int(row["mapq"]), cigar="" if row["cigar"] == "*" else row["cigar"], seq=row["seq"], qual=row["qual"])
        mapped = row["as_bits"] != "*"
        assert mapped == (want["cigar"] != "") == (not want["flags"] & 0x4)
    cmp("name", got["name"], inp["name"])
    for k, v in want.items():
        cmp(k, got[k] & flag_mask if k == "flags" else got[k], v & flag_mask if k == "flags" else v)
    new = {}
    if mapped:
        new = {"AS": ("f", int(row["as_bits"], 16)), "NM": ("i", int(row["nm"])), "MD": ("Z", row["md"]), "X0": ("i", int(row["x0"])), "X1": ("i", int(row["x1"])), "XT": ("A", row["xt"])}
        if row["xa"] != "*":
            new["XA"] = ("Z", row["xa"])
        if row["xs_bits"] != "*":
            new["XS"] = ("f", int(row["xs_bits"], 16))
    for t in NEW_TAG_ORDER[:-1]:
        g = tags.get(t)
        if g is not None and g[0] == "f":
            g = ("f", _f32_bits(g[1]))
        cmp(t, g, new.get(t))
    for t, ty, val in kept:
        cmp("input_tag", tags.get(t), (ty, val))
    cmp("other_tags", sorted(set(tags) - set(new) - {t[0] for t in kept} - {"XD"}), [])
    if "tag_order" in got:
        cmp("tag_order", [t for t in got["tag_order"] if t not in drop_tags], [t[0] for t in kept] + [t for t in NEW_TAG_ORDER if t in new or t == "XD"])
        cmp("bin", got["bin"], reg2bin(want["pos"], want["pos"] + ref_len(want["cigar"])) if mapped else 4680)
        cmp("mate", (got["next_tid"], got["next_pos"], got["tlen"]), (-1, -1, 0))
    return bad


def compare(got, rows, recs, **kw):
    """every record of a run against its expectation -> (number of records that differ, the first of them with their fields, records that differ by field)"""
    assert len(got) == len(rows) == len(recs), (len(got), len(rows), len(recs))
    n_bad, first, per_field = 0, [], {}
    for i, (g, row, inp) in enumerate(zip(got, rows, recs)):
        bad = differing_fields(g, row, inp, **kw)
        if bad:
            n_bad += 1
            if len(first) < 10:
                first.append((i, inp["name"], bad))
            for f in bad:
                per_field[f] = per_field.get(f, 0) + 1
    return n_bad, first, per_field


def report(n, n_bad, first, per_field, what=""):
    return f"{what}: {n_bad} of {n} records differ; the first: {first}; records that differ by field: {per_field}"


def host_record(r, inp):
    """a record dict of mapad_amd.hits_to_records as the writer would lay it out (mapping.rs:795-819: SEQ reversed and complemented, QUAL reversed on the reverse strand)"""
    rev = r["mapped"] and r["reverse"]
    tags = {}
    if r["mapped"]:
        tags = {"AS": ("f", float(r["as"])), "NM": ("i", r["nm"]), "MD": ("Z", r["md"]), "X0": ("i", r["x0"]), "X1": ("i", r["x1"]), "XT": ("A", r["xt"])}
        if r["xa"]:
            tags["XA"] = ("Z", r["xa"])
        if r["xs"] is not None:
            tags["XS"] = ("f", float(r["xs"]))
    for t, ty, val in inp["tags"]:  # copied by the writer, which the host path does not reach
        if t not in MAPPER_TAGS:
            tags[t] = (ty, val)
    return dict(name=inp["name"], flags=r["flags"], tid=r["tid"], pos=r["pos"], mapq=r["mapq"], cigar=r["cigar"], seq=revcomp(inp["seq"]) if rev else inp["seq"],
                qual=inp["qual"][::-1] if rev else inp["qual"], tags=tags)


# ---- reach ----------------------------------------------------------------------------------------------------------------------------------------------------
def view_of_row(row):
    m = row["as_bits"] != "*"
    return dict(mapped=m, flags=int(row["flags"]), tid=int(row["tid"]), pos=int(row["pos"]), mapq=int(row["mapq"]), cigar=row["cigar"], xa=m and row["xa"] != "*", x0=int(row["x0"]) if m else 0)


def view_of_bam(g):
    m = not g["flags"] & 0x4
    return dict(mapped=m, flags=g["flags"], tid=g["tid"], pos=g["pos"], mapq=g["mapq"], cigar=g["cigar"], xa="XA" in g["tags"], x0=g["tags"]["X0"][1] if m else 0)


def reach_counts(views, recs):
    """views: one per input record (view_of_row / view_of_bam; the records that cannot be mapped may be None).  The counts that check_reach() holds to conditions, over the 2240 base reads,
    then what the whole input is there for: every input flag value among mapped and unmapped outputs, 0x10 inputs that map to the reverse strand, and the duplicates
    whose copy lands on another position than its original (the run index reaches PrRange)."""
    base = [v for v, r in zip(views, recs) if r["base"]]
    m = [v for v in base if v["mapped"]]
    by_name = {r["name"]: v for v, r in zip(views, recs)}
    pairs = [(by_name[r["copy_of"]], v) for v, r in zip(views, recs) if r["copy_of"]]
    both = [(a, b) for a, b in pairs if a["mapped"] and b["mapped"]]
    live = [(v, r) for v, r in zip(views, recs) if v is not None]
    return dict(base_reads=len(base), mapped=len(m), unmapped=len(base) - len(m), mapq_le_3=sum(v["mapq"] <= 3 for v in m), mapq_4_36=sum(4 <= v["mapq"] <= 36 for v in m),
                with_xa=sum(v["xa"] for v in m), x0_ge_3=sum(v["x0"] >= 3 for v in m), x0_ge_300=sum(v["x0"] >= 300 for v in m),
                gapped=sum("I" in v["cigar"] or "D" in v["cigar"] for v in m), reverse_share=sum(bool(v["flags"] & 0x10) for v in m) / max(len(m), 1),
                tids=sorted({v["tid"] for v in m}),
                in_flags_mapped=sorted({r["flags"] for v, r in live if v["mapped"]}), in_flags_unmapped=sorted({r["flags"] for v, r in live if not v["mapped"]}),
                out_0x100_or_0x800=sum(bool(v["flags"] & 0x900) for v, _ in live),
                reverse_from_0x10=sum(v["mapped"] and bool(v["flags"] & 0x10) and bool(r["flags"] & 0x10) for v, r in live),
                copies=len(pairs), copies_of_x0_ge_3=sum(a["x0"] >= 3 for a, _ in pairs), copies_elsewhere=sum((a["tid"], a["pos"]) != (b["tid"], b["pos"]) for a, b in both))


def check_reach(c):
    """Conditions, not measurements: each count at about half of what the oracle's expectation of the 2240 base reads yields under the damage preset (mapped 1612, unmapped
    628, MAPQ <= 3: 479, MAPQ 4..36: 196, XA 552, X0 >= 3: 440, X0 >= 300: 97, gapped 74, reverse share 0.47, all four contigs)"""
    assert c["base_reads"] == 2240 and c["mapq_le_3"] >= 240 and c["mapq_4_36"] >= 95 and c["with_xa"] >= 270 and c["x0_ge_3"] >= 220 and c["x0_ge_300"] >= 45 and c["gapped"] >= 35, c
    assert c["reverse_share"] > 0.3 and c["tids"] == [0, 1, 2, 3], c
    assert c["in_flags_mapped"] == c["in_flags_unmapped"] == sorted(IN_FLAGS) and c["out_0x100_or_0x800"] == 0 and c["reverse_from_0x10"] >= 1, c
    assert c["copies"] == N_DUPLICATES and c["copies_of_x0_ge_3"] >= 100 and c["copies_elsewhere"] >= 100, c


def expected_duplicates(rows):
    """per row: does its (tid, POS, reference span, strand) repeat that of an earlier mapped row?  (first in input order is the original)"""
    seen, out = set(), []
    for row in rows:
        if row is None or row["as_bits"] == "*":
            out.append(False)
            continue
        key = (row["tid"], row["pos"], ref_len(row["cigar"]), int(row["flags"]) & 0x10)
        out.append(key in seen)
        seen.add(key)
    return out
