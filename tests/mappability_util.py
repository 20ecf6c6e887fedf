"""The mappability rule restated in plain Python, and the case table the host and the GPU tests share.

The rule reads the INDEX's text, not the FASTA: the text is recovered from the BWT (mapad_index_copy_bwt) by LF walks, so a short ambiguity run is the bases the
index drew for it and a long one is 'X'.  size(N) = occurrences of N in forward + '$' + reverse complement + '$'; loci(N) = size(N), halved when N is its own
reverse complement; c(p) = sum of loci over the k-mer at p and, with e = 1, its 3k neighbours at Hamming distance 1, stored as min(c, 255); 0 for a start
whose k-mer leaves the contig or has anything but A, C, G, T (either case) in the caller's sequence.
"""
import functools
from collections import Counter

import numpy as np

import mapad_amd

SYMS = "$ACGTX"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "X": "X"}
KS = (1, 2, 5, 16, 31, 32, 33, 35, 64, 255)
BINS = ((1, 1), (2, 2), (3, 4), (5, 8), (9, 16), (17, 32), (33, 64), (65, 128), (129, 1 << 62))


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def index_text(index):
    """The two halves of the index's text (each without its '$'), from the BWT alone: rows 0 and 1 are the two suffixes that start with '$'; walking LF from either
    spells the half in front of it backwards.  One is the forward strand, the other its reverse complement — every count of the rule is symmetric in the two."""
    bwt = index.bwt().astype(np.int64)
    less = np.concatenate(([0], np.cumsum(np.bincount(bwt, minlength=6))))
    rank = np.zeros(bwt.size, np.int64)
    for sym in range(6):
        rows = np.flatnonzero(bwt == sym)
        rank[rows] = np.arange(rows.size)
    halves = []
    for row in (0, 1):
        out = []
        while bwt[row] != 0:
            out.append(SYMS[bwt[row]])
            row = less[bwt[row]] + rank[row]
        halves.append("".join(reversed(out)))
    assert len(halves[0]) == len(halves[1]) == (bwt.size - 2) // 2 and halves[1] == revcomp(halves[0])
    return halves


def kmer_sizes(halves, k):
    """size(N) for every N that occurs: windows of both halves (a window with 'X' in it is no string over ACGT and is never asked for)"""
    c = Counter()
    for h in halves:
        for i in range(len(h) - k + 1):
            c[h[i:i + k]] += 1
    return c


def rule_counts(sizes, seq, k, e):
    seq = seq.upper()
    out = np.zeros(len(seq), np.uint8)

    def loci(n):
        s = sizes.get(n, 0)
        return s // 2 if n == revcomp(n) else s

    for p in range(len(seq) - k + 1):
        kmer = seq[p:p + k]
        if any(ch not in "ACGT" for ch in kmer):
            continue
        total = loci(kmer)
        if e:
            for j in range(k):
                for b in "ACGT":
                    if b != kmer[j]:
                        total += loci(kmer[:j] + b + kmer[j + 1:])
        out[p] = min(total, 255)
    return out


def rule_cover(counts, k):
    return np.array([int((counts[max(0, x - k + 1):x + 1] == 1).sum()) for x in range(len(counts))], np.uint8).reshape(-1)


def possible(x, k, length):
    return sum(1 for s in range(max(0, x - k + 1), x + 1) if s + k <= length)


def rule_masks(counts, cover, k):
    length = len(counts)
    poss = np.array([possible(x, k, length) for x in range(length)], np.int64).reshape(-1)
    cov = cover.astype(np.int64)
    return {"start": counts == 1, "majority": 2 * cov > poss, "strict": (poss > 0) & (cov == poss)}


def rule_figures(counts, cover, k):
    m = rule_masks(counts, cover, k)
    valid = counts[counts > 0].astype(np.int64)
    return {"length": len(counts), "valid_starts": int(valid.size), "unique_starts": int((counts == 1).sum()),
            "hist": [int(((valid >= lo) & (valid <= hi)).sum()) for lo, hi in BINS], "majority": int(m["majority"].sum()), "strict": int(m["strict"].sum())}


def add_figures(rows):
    tot = {key: sum(r[key] for r in rows) for key in ("length", "valid_starts", "unique_starts", "majority", "strict")}
    tot["hist"] = [sum(r["hist"][b] for r in rows) for b in range(len(BINS))]
    return tot


def runs(values):
    """[(start, end, value)] of the maximal runs of equal values"""
    out, start = [], 0
    for x in range(1, len(values) + 1):
        if x == len(values) or values[x] != values[start]:
            out.append((start, x, values[start]))
            start = x
    return out if len(values) else []


def rule_bed(names, masks):
    return "".join(f"{name}\t{a}\t{b}\n" for name, m in zip(names, masks) for a, b, v in runs(list(m)) if v)


def rule_bedgraph(names, counts):
    return "".join(f"{name}\t{a}\t{b}\t{int(v)}\n" for name, c in zip(names, counts) for a, b, v in runs(list(c)))


def rule_report(names, rows, k, e):
    head = "contig\tlength\tvalid_starts\tunique_starts\tc1\tc2\tc3_4\tc5_8\tc9_16\tc17_32\tc33_64\tc65_128\tc129_up\tmajority\tstrict\n"

    def line(name, r):
        return "\t".join([name] + [str(v) for v in [r["length"], r["valid_starts"], r["unique_starts"]] + r["hist"] + [r["majority"], r["strict"]]]) + "\n"

    return f"#k\t{k}\n#max_mismatches\t{e}\n" + head + "".join(line(n, r) for n, r in zip(names, rows)) + line("total", add_figures(rows))


# ---- the case table ----------------------------------------------------------------------------------------------------------------------------------
def rand_seq(n, seed):
    return "".join(np.random.RandomState(seed).choice(list("ACGT"), n))


def _planted():
    s = list(rand_seq(300, 11))
    s[120:160] = s[10:50]                              # an exact 40 bp repeat
    s[170:210] = list(revcomp("".join(s[60:100])))     # a reverse-complement repeat
    s[255:295] = s[10:50]                              # a copy with one substitution
    s[275] = "A" if s[275] != "A" else "C"
    return "".join(s)


def _palindromes(twice):
    s = rand_seq(70, 21) + "GAATTC" + rand_seq(40, 22) + "AT" + rand_seq(30, 23) + "GAATTG" + rand_seq(30, 24)  # GAATTG: one substitution away from a palindrome
    return s + ("GAATTC" + rand_seq(25, 25) if twice else "")


def _ambiguous():
    s = rand_seq(100, 31) + "NRN" + rand_seq(60, 32) + "N" * 25 + rand_seq(60, 33)
    return s[:40] + s[40:80].lower() + s[80:]


# name -> (contigs [(name, sequence)], the values of k).  e = 0 and 1 for k <= 35, e = 0 above.
CASES = {
    "planted": ([("chrP", _planted())], KS),
    "three_contigs": ([("a", rand_seq(120, 41)), ("short", rand_seq(20, 42)), ("exact", rand_seq(35, 43))], (16, 35)),
    "palindrome_once": ([("pal1", _palindromes(False))], (2, 5, 6, 7)),
    "palindrome_twice": ([("pal2", _palindromes(True))], (2, 6)),
    "saturation": ([("sat", "A" * 400 + "T" * 150)], (4,)),
    "ambiguous": ([("amb", _ambiguous())], (5, 16, 35)),
    "text47": ([("t47", rand_seq(47, 51))], (1, 5, 16)),   # n = 2 |G| + 2 = 96: the last row is the last of a 96-row block
    "text48": ([("t48", rand_seq(48, 52))], (1, 5, 16)),   # 98
    "text95": ([("t95", rand_seq(95, 53))], (1, 5, 16)),   # 192
}
PARAMS = [(name, k, e) for name, (_, ks) in CASES.items() for k in ks for e in ((0, 1) if k <= 35 else (0,))]
WINDOWS = ((0, 50), (37, 101), (240, 60), (300, 0), (123, 0))  # of "planted": at 0, unaligned in the middle, at the contig's end, empty


@functools.lru_cache(maxsize=None)
def case_index(name):
    contigs = CASES[name][0]
    return mapad_amd.Index.build([(n, s.encode()) for n, s in contigs])


@functools.lru_cache(maxsize=None)
def case_text(name):
    return tuple(index_text(case_index(name)))


@functools.lru_cache(maxsize=None)
def expected(name, k, e):
    """per contig (counts, cover) by the rule; computed once, shared by every test: treat as read-only"""
    sizes = kmer_sizes(case_text(name), k)
    out = []
    for _, seq in CASES[name][0]:
        c = rule_counts(sizes, seq, k, e)
        c.setflags(write=False)
        v = rule_cover(c, k)
        v.setflags(write=False)
        out.append((c, v))
    return tuple(out)


def expected_figures(name, k, e):
    return [rule_figures(c, v, k) for c, v in expected(name, k, e)]


def write_reference(name, path):
    """the case's FASTA (60 columns) and its index beside it, as `mapad-amd mappability -g` wants them"""
    with open(path, "w") as f:
        for n, s in CASES[name][0]:
            f.write(f">{n} some description\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    case_index(name).save(str(path))


def expected_files(name, k, e):
    names = [n for n, _ in CASES[name][0]]
    exp = expected(name, k, e)
    files = {"bedgraph": rule_bedgraph(names, [c for c, _ in exp]), "report": rule_report(names, expected_figures(name, k, e), k, e)}
    for rule in ("start", "majority", "strict"):
        files[rule] = rule_bed(names, [rule_masks(c, v, k)[rule] for c, v in exp])
    return files


def run_cli_files(cli, fasta, tmp_path, k, e, extra=()):
    """mapad-amd mappability once per BED rule: {"start" | "majority" | "strict" | "bedgraph" | "report": file text}"""
    import subprocess
    out = {}
    for rule in ("start", "majority", "strict"):
        bed, bg, rep = (str(tmp_path / f"{rule}.{ext}") for ext in ("bed", "bedgraph", "tsv"))
        subprocess.run([cli, "mappability", "-g", str(fasta), "-k", str(k), "--max_mismatches", str(e), "--bed", bed, "--bed_rule", rule, "--bedgraph", bg, "--report", rep,
                        *extra], check=True, capture_output=True, timeout=120)
        out[rule] = open(bed).read()
        out["bedgraph"], out["report"] = open(bg).read(), open(rep).read()
    return out
