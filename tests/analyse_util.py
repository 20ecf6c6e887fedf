"""Tracks from alignments computed independently of the product: what mapad_amd/csrc/align_core.hpp makes of (CIGAR, MD, read length, strand) written once more
in plain Python — MD expanded per reference position, the CIGAR walked column by column, the operation words packed as a search's track carries them —, the
table of shapes both tests/test_analyse_host.py (the host path) and tests/test_gpu_analyse.py (the device against the host) run, random consistent alignments,
and the conversion of the library's records into the arrays mapad_ctx_accumulate_alignments takes."""
import re

import numpy as np

import mapad_amd
from mapad_amd import binding as mb

OP_INS, OP_DEL, OP_MATCH, OP_MISMATCH = 0, 1, 2, 3
CLASSES = mb.ALN_CLASSES
CLS = {k: i for i, k in enumerate(CLASSES)}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H", "H": "D"}
_MD = re.compile(r"(\d+)|\^([A-Za-z]+)|([A-Za-z])")
_CIGAR = re.compile(r"(\d+)([MIDNSHP=X])")
SMALL = [3_000, 2_000]  # contig lengths of the CPU tests' index (a track does not depend on the bases)


def cigar_ops(cigar):
    return [(int(n), op) for n, op in _CIGAR.findall(cigar)]


def expected_track(cigar, md, L, reverse, start_at_end=True):
    """-> the track's words in track order (read order), or None where MD cannot be parsed or disagrees with the CIGAR"""
    ref, at = [], 0  # per reference position: None = match, ("X", base), ("D", base)
    for m in _MD.finditer(md):
        if m.start() != at:
            return None
        at = m.end()
        if m.group(1) is not None:
            if len(m.group(1)) > 10 or int(m.group(1)) > 65535:
                return None
            ref += [None] * int(m.group(1))
        elif m.group(2) is not None:
            ref += [("D", b.upper()) for b in m.group(2)]
        else:
            ref.append(("X", m.group(3).upper()))
    if at != len(md):
        return None
    cols, s, x = [], 0, 0  # (kind, reference base, index in SEQ) in reference order
    for n, op in cigar_ops(cigar):
        for _ in range(n):
            if op == "I":
                cols.append((OP_INS, None, s))
                s += 1
            elif op == "D":
                if x >= len(ref) or ref[x] is None or ref[x][0] != "D":
                    return None
                cols.append((OP_DEL, ref[x][1], s))
                x += 1
            else:
                if x >= len(ref) or (ref[x] is not None and ref[x][0] == "D"):
                    return None
                cols.append((OP_MATCH, None, s) if ref[x] is None else (OP_MISMATCH, ref[x][1], s))
                s += 1
                x += 1
    if x != len(ref):
        return None
    start = L if start_at_end else L // 2
    words = []
    for kind, b, s in cols:
        base = 0 if b is None else ord(_COMP.get(b, b) if reverse else b)
        if kind == OP_DEL:
            q = L - s if reverse else s  # read bases in front of the deletion in read order
            p = (q - 1 if q else 0) if q <= start else q
            p = min(p, L - 1)
        else:
            p = L - 1 - s if reverse else s
        words.append(kind << 24 | base << 16 | p)
    return words[::-1] if reverse else words


def expected_class(rec, L, lengths, min_mapq=0, start_at_end=True):
    """the first class that applies, in the order the issue lists them"""
    if rec.get("flags", 0) & 0x4 or rec["tid"] < 0 or rec["pos"] < 0:
        return CLS["unmapped"]
    if rec.get("mapq", 0) < min_mapq:
        return CLS["below_min_mapq"]
    if not rec.get("md"):
        return CLS["no_md"]
    if rec["tid"] >= len(lengths):
        return CLS["bad_contig"]
    ops = cigar_ops(rec["cigar"] or "")
    if not ops or any(op in "SHNP" for _, op in ops):
        return CLS["unsupported_cigar"]
    if sum(n for n, op in ops if op in "MI=X") != L:
        return CLS["length_mismatch"]
    if expected_track(rec["cigar"], rec["md"], L, bool(rec.get("flags", 0) & 0x10), start_at_end) is None:
        return CLS["md_mismatch"]
    span = sum(n for n, op in ops if op in "MD=X")
    if rec["pos"] >= lengths[rec["tid"]] or rec["pos"] + span > lengths[rec["tid"]]:
        return CLS["off_contig"]
    return CLS["ok"]


def _rec(cigar, md, tid=0, pos=100, reverse=False, mapq=37, x0=1, score=-1.5, flags=0):
    return {"tid": tid, "pos": pos, "flags": flags | (0x10 if reverse else 0), "mapq": mapq, "x0": x0, "as": score, "cigar": cigar, "md": md}


def shapes(lengths):
    """[(name, record, read length)]: the shapes of the issue's table on contigs of the given lengths, each on either strand"""
    n1 = lengths[0]
    out = []

    def both(name, cigar, md, L, **kw):
        for rev in (False, True):
            out.append((f"{name}{'-' if rev else '+'}", _rec(cigar, md, reverse=rev, **kw), L))

    both("all-match", "50M", "50", 50)
    both("mismatch in the first column", "30M", "0A29", 30)
    both("mismatch in the first column, no leading zero", "30M", "A29", 30)
    both("mismatch in the last column", "30M", "29C0", 30)
    both("two mismatches with a zero between", "17M", "10A0C5", 17)
    both("deletion, zero, mismatch", "5M2D4M", "5^AC0T3", 9)
    both("three-base deletion", "20M3D20M", "20^ACG20", 40, x0=3)
    both("insertion in front of a deletion", "10M2I3D10M", "10^TTT10", 22)
    both("deletion in front of an insertion", "10M3D2I10M", "10^GCA10", 22)
    both("= and X that contradict MD", "5=1X4=", "10", 10)
    both("= where MD has a mismatch", "10=", "4G5", 10)
    both("lower-case MD", "10M", "4g5", 10)
    both("lower-case deletion", "3M2D4M", "3^ac4", 7)
    both("N in MD", "10M", "5N4", 10)
    both("an ambiguity code in MD", "10M", "2R7", 10)
    both("no X0", "12M", "12", 12, x0=None)
    for L in (1, 63, 64, 65, 129):
        both(f"length {L}", f"{L}M", str(L), L)
        both(f"length {L}, last column", f"{L}M", f"{L - 1}T0", L)
    both("more than 64 CIGAR operations", "1M1I" * 100, "100", 200)
    both("more than 64 CIGAR operations, mismatches", "1M1I" * 100, "0A" + "9C" * 9 + "9", 200)
    both("a deletion that straddles column 64", "62M5D30M", "62^ACGTA30", 92)
    both("a deletion at column 64", "64M2D1M", "64^GG1", 65)
    both("zero-length operations", "0M5M0I0D5M", "10", 10)
    both("the last base of a contig", "25M", "25", 25, pos=n1 - 25)
    both("the first base of the second contig", "25M", "0C24", 25, tid=1, pos=0)
    both("the last base of the last contig", "10M1D5M", "10^A5", 15, tid=1, pos=lengths[1] - 16)
    # wider than one window of the build kernel, MD longer than one trip
    md = "".join(f"17{'ACGT'[k & 3]}" for k in range(40)) + "6^" + "ACGTT" * 14 + "13"  # 40 * 18 + 6 = 726 columns, 70 deleted bases, 13 columns
    both("several windows and MD trips", "300M1I426M70D13M", md, 740)
    # ten inserted bases: the column trip from column 256 on begins at offset 246, inside the first window, behind an MD trip of exactly 64 bytes that ends at 251
    both("a window that begins inside the one before", "10M10I300M", "7A" * 30 + "9C" + "0G" + "59", 320)
    # one read per class, each with later classes' faults too: the class is the FIRST that applies
    out += [("unmapped", _rec("10M", None, flags=0x4, mapq=0), 10), ("unmapped by tid", _rec("10M", "10", tid=-1), 10), ("unmapped by pos", _rec("10M", "10", pos=-1), 10),
            ("below_min_mapq", _rec("5S5M", None, mapq=5, tid=9), 10), ("no_md", _rec("5S5M", None, tid=9), 10), ("no_md, empty", _rec("10M", ""), 10),
            ("bad_contig", _rec("5S5M", "7", tid=len(lengths)), 12), ("unsupported_cigar S", _rec("5S5M", "7"), 12), ("unsupported_cigar H", _rec("5H10M", "10"), 10),
            ("unsupported_cigar N", _rec("5M100N5M", "10"), 10), ("unsupported_cigar P", _rec("5M1P5M", "10"), 10), ("unsupported_cigar none", _rec("", "10"), 10),
            ("length_mismatch", _rec("10M", "9", pos=n1 - 5), 12), ("length_mismatch with I", _rec("5M2I5M", "10"), 10),
            ("md_mismatch short", _rec("10M", "9", pos=n1 - 5), 10), ("md_mismatch long", _rec("10M", "11"), 10), ("md_mismatch deletion without D", _rec("10M", "4^A5"), 10),
            ("md_mismatch D without deletion", _rec("5M1D5M", "11"), 10), ("md_mismatch D on a mismatch", _rec("5M1D5M", "5A5"), 10),
            ("md_mismatch character", _rec("10M", "5?4"), 10), ("md_mismatch bare ^", _rec("10M", "5^5"), 10), ("md_mismatch ^ at the end", _rec("10M", "10^"), 10),
            ("md_mismatch long number", _rec("10M", "00000000010"), 10), ("md_mismatch large number", _rec("10M", "70000"), 10),
            ("off_contig", _rec("10M", "10", pos=n1 - 5), 10), ("off_contig by a deletion", _rec("5M1D5M", "5^A5", pos=n1 - 10), 10),
            ("off_contig at the end", _rec("10M", "10", pos=n1), 10)]
    return out


def random_alignments(rng, n, lengths, len_range=(1, 300), reverse_frac=0.5):
    """n consistent alignments with mismatches, insertions and deletions, placed inside the contigs -> [(record, read length)]"""
    out = []
    for _ in range(n):
        L = int(rng.integers(len_range[0], len_range[1] + 1))
        ops, md, run, left, prev = [], "", 0, L, None
        while left:
            kind = rng.choice(["M", "M", "M", "I", "D"]) if prev == "M" else "M"
            k = int(rng.integers(1, 5)) if kind != "M" else int(rng.integers(1, min(left, 90) + 1))
            if kind == "I":
                k = min(k, left)
                left -= k
            elif kind == "D":
                md += f"{run}^" + "".join(rng.choice(list("ACGT"), k))
                run = 0
            else:
                left -= k
                for _ in range(k):
                    if rng.random() < 0.08:
                        md += f"{run}" + str(rng.choice(list("ACGTNacgt")))
                        run = 0
                    else:
                        run += 1
            ops.append((k, kind))
            prev = kind
        md += str(run)
        if ops[-1][1] == "D":  # (an alignment does not end in a deletion; MD would need a number behind it anyway)
            ops.append((0, "M"))
        cigar = "".join(f"{k}{op}" for k, op in ops)
        span = sum(k for k, op in ops if op != "I")
        tid = int(rng.integers(0, len(lengths)))
        pos = int(rng.integers(0, lengths[tid] - span + 1))
        out.append((_rec(cigar, md, tid=tid, pos=pos, reverse=bool(rng.random() < reverse_frac), mapq=int(rng.integers(0, 38)), x0=int(rng.integers(1, 4))), L))
    return out


def offsets_of(read_lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(read_lengths, np.uint64))]).astype(np.uint64)


def assert_tracks(t, recs, read_lengths, lengths, min_mapq=0, start_at_end=True, names=None):
    """t: what alignment_tracks_host / Context.alignment_tracks return -> every array against the Python rule above"""
    n = len(recs)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    assert np.array_equal(t["hit_begin"], np.arange(n + 1, dtype=np.uint64))
    reserved = 0
    counts = {k: 0 for k in CLASSES}
    for r, (rec, L) in enumerate(zip(recs, read_lengths)):
        what = (names[r] if names else r, rec)
        cls = expected_class(rec, L, lengths, min_mapq, start_at_end)
        counts[CLASSES[cls]] += 1
        assert t["status_class"][r] == cls, (what, CLASSES[t["status_class"][r]], CLASSES[cls])
        h = t["hits"][r]
        assert h["lower"] == 0 and h["lower_rev"] == 0 and h["reserved"] == 0 and h["ops_offset"] == reserved, what
        assert t["best"][r] == 0 and t["error"][r] == 0, what
        if cls == CLS["ok"]:
            want = expected_track(rec["cigar"], rec["md"], L, bool(rec["flags"] & 0x10), start_at_end)
            got = t["ops"][reserved:reserved + int(h["n_ops"])]
            assert list(got) == want, (what, [hex(w) for w in got[:8]], [hex(w) for w in want[:8]])
            x0 = rec["x0"] or 1
            assert h["size"] == x0 and h["score"] == np.float32(rec["as"]) and t["x0"][r] == x0, what
            assert (t["mapped"][r], t["tid"][r], t["rel"][r], t["abs"][r], t["backward"][r]) == (1, rec["tid"], rec["pos"], starts[rec["tid"]] + rec["pos"], rec["flags"] >> 4 & 1), what
        else:
            assert h["n_ops"] == 0 and h["size"] == 0 and h["score"] == 0 and t["mapped"][r] == 0 and t["x0"][r] == 0 and t["tid"][r] == -1, what
        # a read keeps the room its CIGAR asks for whenever the CIGAR-only classes let it pass
        if cls in (CLS["ok"], CLS["md_mismatch"], CLS["off_contig"]):
            reserved += sum(k for k, op in cigar_ops(rec["cigar"]) if op in "MIDX=")
    assert len(t["ops"]) == reserved and t["class_counts"] == counts, (t["class_counts"], counts)
    return counts


def same_tracks(a, b):
    """two track dicts bit for bit, the unwritten room of the reads that failed late excepted"""
    for k in ("hit_begin", "status_class", "mapped", "error", "best", "x0", "tid", "rel", "abs", "backward"):
        assert np.array_equal(a[k], b[k]), k
    assert a["hits"].tobytes() == b["hits"].tobytes() and a["class_counts"] == b["class_counts"] and len(a["ops"]) == len(b["ops"])
    keep = np.zeros(len(a["ops"]), bool)
    for h in a["hits"]:
        keep[int(h["ops_offset"]):int(h["ops_offset"]) + int(h["n_ops"])] = True
    assert np.array_equal(a["ops"][keep], b["ops"][keep])


def alignments_of(recs, mapq=None):
    """the library's decoded records (hits_to_records) -> the arrays accumulate_alignments takes"""
    rows = []
    for i, r in enumerate(recs):
        rows.append({"tid": r["tid"], "pos": r["pos"], "flags": r["flags"], "mapq": r["mapq"] if mapq is None else int(mapq[i]), "x0": r["x0"] if r["mapped"] else None,
                     "as": float(r["as"]) if r["mapped"] else 0.0, "cigar": r["cigar"] if r["mapped"] else "", "md": r["md"] if r["mapped"] else None})
    return mapad_amd.pack_alignments(rows)


def write_aligned_bam(path, header_text, refs, records):
    """records: dicts name, flags, tid, pos, mapq, cigar (text), seq, qual (Phred+33), tags [(tag, type Z | i | f | A, value)] -> a BAM with their alignment fields
    (bam_util.write_bam writes unaligned records only)"""
    import struct

    from bam_util import _CODE, _bgzf_block
    out = b"BAM\x01" + struct.pack("<i", len(header_text)) + header_text.encode() + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    for r in records:
        seq, name = r["seq"], r["name"].encode() + b"\0"
        words = [n << 4 | "MIDNSHP=X".index(op) for n, op in cigar_ops(r.get("cigar") or "")]
        packed = bytes(_CODE.index(seq[i]) << 4 | (_CODE.index(seq[i + 1]) if i + 1 < len(seq) else 0) for i in range(0, len(seq), 2))
        aux = b""
        for tag, ty, val in r.get("tags", []):
            aux += tag.encode() + ty.encode() + {"Z": lambda v: v.encode() + b"\0", "i": lambda v: struct.pack("<i", v), "f": lambda v: struct.pack("<f", v),
                                                 "A": lambda v: v.encode()}[ty](val)
        body = struct.pack("<iiBBHHHiiii", r.get("tid", -1), r.get("pos", -1), len(name), r.get("mapq", 0), 4680, len(words), r["flags"], len(seq), -1, -1, 0) + name + \
            struct.pack(f"<{len(words)}I", *words) + packed + bytes(ord(c) - 33 for c in r["qual"]) + aux
        out += struct.pack("<i", len(body)) + body
    with open(path, "wb") as f:
        for i in range(0, len(out), 60000):
            f.write(_bgzf_block(out[i:i + 60000]))
        f.write(_bgzf_block(b""))
