"""A numpy restatement of the index products (src/index/indexing.rs:163-195) that shares no code with the library or with the oracle: the rank text of
text$revcomp$, its suffix array by plain prefix doubling over np.lexsort, and from it the BWT, the 1/32 SA sample with its extra rows, `less` and the two
sentinel rows — plus the texts that tests/test_index_host.py (host SA-IS) and tests/test_gpu_index_chunks.py (GPU builder with lowered limits) share.

Only texts whose ambiguous runs are 20 or more bases long belong here: those become X deterministically, no random replacement is involved."""
import functools

import numpy as np

from mapad_amd import synth

SA_RATE = 32
_RANK = np.zeros(256, np.uint8)
for _k, _c in enumerate(b"ACGTX"):
    _RANK[_c] = _k + 1


def rank_text(contigs):
    """text $ revcomp(text) $ as ranks ($=0 A=1 C=2 G=3 T=4 X=5) of the concatenated contigs: upper-cased, N -> X; the complement of rank r is 5 - r, X stays X."""
    raw = np.frombuffer(b"".join(bytes(s) for _, s in contigs).upper().replace(b"N", b"X"), dtype=np.uint8)
    fwd = _RANK[raw]
    assert (fwd > 0).all(), "only A, C, G, T, N belong in these texts"
    rc = np.where(fwd == 5, 5, 5 - fwd)[::-1].astype(np.uint8)
    zero = np.zeros(1, np.uint8)
    return np.concatenate([fwd, zero, rc, zero])


def suffix_array(t):
    """Prefix doubling: order by (rank[i], rank[i + h]), positions past the end rank -1 (the shorter suffix sorts first); O(n log^2 n)."""
    t = np.asarray(t)
    n = len(t)
    rank = t.astype(np.int64)
    h = 1
    while True:
        second = np.full(n, -1, np.int64)
        second[:n - h] = rank[h:]
        order = np.lexsort((second, rank))
        r1, r2 = rank[order], second[order]
        new_group = np.ones(n, bool)
        new_group[1:] = (r1[1:] != r1[:-1]) | (r2[1:] != r2[:-1])
        dense = np.cumsum(new_group) - 1
        if dense[-1] == n - 1:
            return order.astype(np.uint64)
        rank = np.empty(n, np.int64)
        rank[order] = dense
        h *= 2
        assert h < 2 * n


class Products:
    def __init__(self, contigs):
        t = rank_text(contigs)
        n = len(t)
        self.n, self.text = n, t
        self.sa = suffix_array(t)
        sa = self.sa.astype(np.int64)
        self.bwt = t[(sa - 1) % n]  # the row of suffix 0 gets the last symbol (indexing.rs:166)
        self.sample = self.sa[::SA_RATE]
        rows = np.arange(n)
        extra = (self.bwt == 0) & (rows % SA_RATE != 0)  # rows whose LF walk would step over a sentinel (index/mod.rs:112-118)
        self.extra_rows, self.extra_values = rows[extra].astype(np.uint64), self.sa[extra]
        counts = np.bincount(t, minlength=6)
        less = np.zeros(8, np.uint64)
        less[1:7] = np.cumsum(counts[:6])
        less[7] = n
        self.less = less
        self.sentinel = rows[self.bwt == 0].astype(np.uint64)
        assert len(self.sentinel) == 2


def assert_index_equals_reference(ix, ref, what=""):
    """every product of a library index (host- or GPU-built) against the numpy restatement, and the suffix array of ALL rows through the library's LF walk over the rank blocks"""
    assert len(ix) == ref.n, what
    assert np.array_equal(ix.bwt(), ref.bwt), f"{what}: BWT"
    sample, er, ev = ix.sampled_sa()
    assert np.array_equal(sample, ref.sample), f"{what}: SA sample"
    assert np.array_equal(er, ref.extra_rows) and np.array_equal(ev, ref.extra_values), f"{what}: extra rows"
    _, _, less, sent = ix.device_view()
    assert np.array_equal(less, ref.less), f"{what}: less"
    assert np.array_equal(sent, ref.sentinel), f"{what}: sentinel rows"
    got = ix.sa_get_batch(np.arange(ref.n, dtype=np.uint64))
    assert np.array_equal(got, ref.sa), f"{what}: sa_get_batch, first differing row {int(np.argmax(got != ref.sa))}"


# ---- texts ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _g(n, s):
    return synth.genome(n, seed=s).tobytes()


def _mixed():
    u, mix = _g(37, 8), _g(15_000, 9)
    text = mix + u * 400 + mix[:5000] + b"N" * 3000 + mix[5000:9000] + b"AC" * 3000  # unique text, a 37 bp tandem, a 5 kbp copy, an N run, a 4 kbp copy, a dinucleotide run
    return [("a", text[:15_000]), ("b", text[15_000:34_800]), ("c", text[34_800:])]


def _n_runs():
    g = synth.genome(60_000, seed=7).copy()
    for a, b in ((1000, 9000), (20_000, 20_300), (40_000, 47_000), (59_000, 60_000)):
        g[a:b] = ord("N")
    return [("c", g.tobytes())]


def _uniform(n):
    rng = np.random.default_rng(1000 + n)
    return [("c", np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes())]


TEXTS = {
    "mixed": _mixed,                                                   # n = 95 602
    "two_copies_20k": lambda: [("c", _g(20_000, 5) * 2)],              # n = 80 002: every suffix in a group of two
    "n_runs": _n_runs,                                                 # n = 120 002: four X runs, the longest 8 000 (16 000 tied suffixes with the reverse complement's)
    "polyA": lambda: [("c", b"A" * 70_000)],                           # as in test_gpu_index.py
    "tandem": lambda: [("c", b"ACGTTGCA" * 20_000)],
    "uniform3": lambda: _uniform(3), "uniform9": lambda: _uniform(9), "uniform257": lambda: _uniform(257), "uniform4097": lambda: _uniform(4097),
}
TEXT_LEN = {"mixed": 95_602, "two_copies_20k": 80_002, "n_runs": 120_002, "polyA": 140_002, "tandem": 320_002, "uniform3": 8, "uniform9": 20, "uniform257": 516, "uniform4097": 8196}


@functools.lru_cache(maxsize=None)
def contigs(name):
    return TEXTS[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """the numpy products of a text: computed once per process and shared by the tests (treat as read-only)"""
    ref = Products(contigs(name))
    assert ref.n == TEXT_LEN[name]
    for a in (ref.sa, ref.bwt, ref.sample, ref.extra_rows, ref.extra_values, ref.less, ref.sentinel, ref.text):
        a.setflags(write=False)
    return ref
