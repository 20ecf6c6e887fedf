"""What the tests of the device-resident calls (tests/test_gpu_device_io.py on the GPU, tests/test_device_io_host.py without one) share: the HIP runtime through
ctypes — the very file the library has loaded, so that a test owns streams, device buffers and page-locked memory without torch.cuda in the pytest process —, a
stream delay that does not depend on the GPU's speed, the decoder of mapad_records_device's payload (88-byte DevRecord words, text pool, pair pool: the word layout
of mapad_amd/distributed.py) and the pairs a read's mapping quality is computed from, restated from the hit list.

Flags and MAPQ are not in the payload (they are finished on the host, from the pairs and the input flags): decode_device_records leaves both 0, and every
comparison with the oracle's records goes through without_flags_and_mapq() — stated here once."""
import ctypes as C
import time

import numpy as np

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd.distributed import RECORD_WORDS

H2D, D2H, D2D = 1, 2, 3          # hipMemcpyKind
STREAM_NON_BLOCKING = 1          # hipStreamNonBlocking
HIP_SUCCESS, HIP_NOT_READY = 0, 600  # hipErrorNotReady: what hipStreamQuery returns while work is pending
_HOST_FN = C.CFUNCTYPE(None, C.c_void_p)  # hipHostFn_t


def _runtime_path():
    """the libamdhip64 the product library has loaded (a second copy of the runtime would not see its device); a copy that another package brought into the process
    under its own directory (torch ships one) is not it"""
    paths = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln})
    own = [p for p in paths if "/torch/" not in p]
    return (own or paths or ["libamdhip64.so"])[0]


class Hip:
    """The handful of runtime calls the tests need.  Every call is checked; pointers and streams are plain integers."""

    def __init__(self):
        self.lib = mapad_amd.lib()
        h = self.hip = C.CDLL(_runtime_path())
        vp, sz = C.c_void_p, C.c_size_t
        for name, args in {"hipMalloc": [C.POINTER(vp), sz], "hipFree": [vp], "hipMemcpy": [vp, vp, sz, C.c_int], "hipMemcpyAsync": [vp, vp, sz, C.c_int, vp],
                           "hipStreamCreateWithFlags": [C.POINTER(vp), C.c_uint], "hipStreamDestroy": [vp], "hipStreamSynchronize": [vp], "hipStreamQuery": [vp],
                           "hipLaunchHostFunc": [vp, _HOST_FN, vp], "hipDeviceSynchronize": []}.items():
            fn = getattr(h, name)
            fn.restype, fn.argtypes = C.c_int, args
        self.lib.mapad_host_alloc.restype, self.lib.mapad_host_alloc.argtypes = vp, [sz]
        self.lib.mapad_host_free.restype, self.lib.mapad_host_free.argtypes = None, [vp]
        self._callbacks = []  # CFUNCTYPE objects of delays that may not have run yet
        self._device, self._pinned, self._streams = [], [], []

    @staticmethod
    def _ok(rc, what):
        assert rc == HIP_SUCCESS, f"{what} failed with {rc}"

    # ---- memory
    def malloc(self, nbytes):
        p = C.c_void_p()
        self._ok(self.hip.hipMalloc(C.byref(p), max(int(nbytes), 8)), f"hipMalloc of {nbytes} bytes")
        self._device.append(p.value)
        return p.value

    def to_device(self, a, into=None):
        """blocking upload of a numpy array -> device pointer"""
        a = np.ascontiguousarray(a)
        p = self.malloc(a.nbytes) if into is None else into
        if a.nbytes:
            self._ok(self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, H2D), "hipMemcpy to the device")
        return p

    def from_device(self, ptr, n, dtype):
        """blocking copy of n elements -> numpy array"""
        out = np.zeros(int(n), dtype)
        if out.nbytes:
            assert ptr, "a null device pointer for a non-empty array"
            self._ok(self.hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, D2H), "hipMemcpy to the host")
        return out

    def pinned(self, n, dtype=np.uint8):
        """n elements of page-locked host memory from mapad_host_alloc, zeroed -> numpy view (its address: .ctypes.data)"""
        nbytes = max(int(n) * np.dtype(dtype).itemsize, 1)
        p = self.lib.mapad_host_alloc(nbytes)
        assert p, f"mapad_host_alloc of {nbytes} bytes"
        self._pinned.append(p)
        a = np.frombuffer((C.c_char * nbytes).from_address(p), dtype=dtype, count=int(n))
        a[:] = 0
        return a

    def pinned_copy(self, a):
        a = np.ascontiguousarray(a)
        out = self.pinned(a.size, a.dtype)
        out[:] = a.ravel()
        return out

    def copy_async(self, dst, src, nbytes, kind, stream):
        if nbytes:
            self._ok(self.hip.hipMemcpyAsync(dst, src, int(nbytes), kind, stream), "hipMemcpyAsync")

    # ---- streams
    def stream(self):
        s = C.c_void_p()
        self._ok(self.hip.hipStreamCreateWithFlags(C.byref(s), STREAM_NON_BLOCKING), "hipStreamCreateWithFlags")
        self._streams.append(s.value)
        return s.value

    def destroy(self, stream):
        """after the contexts that were given the stream are closed"""
        self.synchronize(stream)
        self._streams.remove(stream)
        self._ok(self.hip.hipStreamDestroy(stream), "hipStreamDestroy")

    def busy(self, stream):
        """True while work queued on the stream has not finished"""
        rc = self.hip.hipStreamQuery(stream)
        assert rc in (HIP_SUCCESS, HIP_NOT_READY), f"hipStreamQuery returned {rc}"
        return rc == HIP_NOT_READY

    def synchronize(self, stream):
        self._ok(self.hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

    def delay(self, stream, seconds):
        """Holds the stream for `seconds`, whatever the GPU's speed: a host function (hipLaunchHostFunc) that sleeps; what is queued behind it on the stream, and
        what waits for an event recorded behind it, starts when it returns.  The function never raises and always returns.  Its CFUNCTYPE object is kept until
        release() — call that only once the stream has been synchronised.  The product library is called through CDLL, which frees the GIL: the runtime's
        callback thread gets it while the main thread sits in a library call that waits for this very stream."""
        def sleep(_):
            try:
                time.sleep(seconds)
            except BaseException:  # noqa: BLE001  (nothing may leave a callback the runtime called)
                pass
        cb = _HOST_FN(sleep)
        self._callbacks.append(cb)
        self._ok(self.hip.hipLaunchHostFunc(stream, cb, None), "hipLaunchHostFunc")

    def release(self):
        """frees what this object handed out (after the contexts that used it are closed); waits for the device first"""
        self._ok(self.hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
        self._callbacks.clear()
        for s in self._streams:
            self.hip.hipStreamDestroy(s)
        for p in self._device:
            self.hip.hipFree(p)
        for p in self._pinned:
            self.lib.mapad_host_free(p)
        self._streams, self._device, self._pinned = [], [], []


# ---- the gather payload -----------------------------------------------------------------------------------------------------------------------------------------
# word indices of a DevRecord (mapad_amd/distributed.py:106-109): i64 pos (0-1), tid 2, mapped 3, reverse 4, as 5, xs 6, nm 7, x0 8, x1 9, has_xs 10, xt 11,
# text_off 12, cigar_len 13, md_len 14, xa_len 15, best_size 16, read_len 17, mq_off 18, mq_n 19, error 20, (padding 21)
RECORD_DTYPE = np.dtype(mb.RecordC)


def decode_device_records(recs_i32, text_u8, pairs_f32):
    """mapad_records_device's three arrays (or merge_gathered_records' merged ones) -> (records in the mapad_record_t field layout that
    hits_to_records(..., as_arrays=True) returns, with flags and mapq 0; the text pool as uint8 — the records' offsets point into it as it is —; and
    dict(pairs=[per read a (mq_n, 2) uint32 array of (score bits, float32(size) bits)], best_size=float32[n], read_len=uint32[n], error=uint32[n])).
    An unmapped read has tid -1, pos -1 and nothing else, like the host path's record."""
    w = np.ascontiguousarray(np.asarray(recs_i32, np.int32)).reshape(-1, RECORD_WORDS)
    u = w.view(np.uint32)
    n = len(w)
    text = np.ascontiguousarray(np.asarray(text_u8)).view(np.uint8).copy()
    pool = np.ascontiguousarray(np.asarray(pairs_f32)).view(np.uint32).reshape(-1, 2)
    m = u[:, 3] != 0
    recs = np.zeros(n, RECORD_DTYPE)
    recs["mapped"] = m
    recs["pos"] = np.where(m, np.ascontiguousarray(w[:, 0:2]).view(np.int64)[:, 0], -1)
    recs["tid"] = np.where(m, w[:, 2], -1)
    recs["reverse"] = np.where(m, u[:, 4], 0)
    recs["as_score"] = np.where(m, u[:, 5], 0).astype(np.uint32).view(np.float32)
    recs["xs_score"] = np.where(m, u[:, 6], 0).astype(np.uint32).view(np.float32)
    for k, name in ((7, "nm"), (8, "x0"), (9, "x1")):
        recs[name] = np.where(m, w[:, k], 0)
    recs["has_xs"] = np.where(m, u[:, 10], 0)
    recs["xt"] = np.where(m, u[:, 11], 0).astype(np.uint8).view("S1")
    off = np.where(m, u[:, 12], 0).astype(np.uint32)
    recs["cigar_off"] = off
    recs["cigar_len"] = np.where(m, u[:, 13], 0)
    recs["md_off"] = off + recs["cigar_len"]
    recs["md_len"] = np.where(m, u[:, 14], 0)
    recs["xa_off"] = recs["md_off"] + recs["md_len"]
    recs["xa_len"] = np.where(m, u[:, 15], 0)
    pairs = [pool[int(o):int(o) + int(k)].copy() if mapped else pool[:0].copy() for mapped, o, k in zip(m, u[:, 18], u[:, 19])]
    extras = dict(pairs=pairs, best_size=u[:, 16].copy().view(np.float32), read_len=u[:, 17].copy(), error=u[:, 20].copy())
    return recs, text, extras


def without_flags_and_mapq(ocanon):
    """the oracle's canonical records (RecordWorld.oracle_canon) with the two fields the payload does not carry set to what decode_device_records leaves: 0"""
    f, texts = ocanon
    f = f.copy()
    f["flags"] = 0
    f["mapq"] = 0
    return f, texts


def _pair_key(p):
    return sorted((int(a), int(b)) for a, b in np.asarray(p, np.uint32).reshape(-1, 2))


def expected_pairs(hits_of_read, reported, remaining=None):
    """The (score, size) pairs behind a read's mapping quality when hit `reported` of its list is the reported one: of its other hits (`remaining`: of those hit
    indices only), those that interval_cross_check does not take for the reported one — same size and (same lower or same lower_rev), the rule of
    records_util.pairs_needed — as a sorted list of (score bits, float32(size) bits): a multiset, the pool's order within a read is the record kernel's own."""
    h = np.asarray(hits_of_read)
    b = h[reported]
    cross = (h["size"] == b["size"]) & ((h["lower"] == b["lower"]) | (h["lower_rev"] == b["lower_rev"]))
    cross[reported] = True
    if remaining is not None:
        out = np.ones(len(h), bool)
        out[np.asarray(remaining, np.int64)] = False
        cross |= out
    keep = h[~cross]
    return _pair_key(np.stack([keep["score"].astype(np.float32).view(np.uint32), keep["size"].astype(np.float32).view(np.uint32)], axis=1))


def sorted_order(scores):
    """Hit indices in the order of BinaryHeap::into_sorted_vec over a heap array of these scores (ascending; Rust's std: swap(0, end), then sift_down_range, which
    takes the right child on ties).  The reference pops hits from the end of this order until one has a coordinate inside a contig (mapping.rs:421-430, :541-543):
    that one is reported, and only the hits in FRONT of it are the `other alignments` of its mapping quality — a hit popped before it no longer counts."""
    s = np.asarray(scores, np.float32)
    d = list(range(len(s)))
    end = len(d)
    while end > 1:
        end -= 1
        d[0], d[end] = d[end], d[0]
        pos, child, elt, placed = 0, 1, d[0], False
        while child + 1 < end:
            if s[d[child]] <= s[d[child + 1]]:
                child += 1
            if s[elt] >= s[d[child]]:
                placed = True
                break
            d[pos] = d[child]
            pos, child = child, 2 * child + 1
        if not placed and child + 1 == end and s[elt] < s[d[child]]:
            d[pos] = d[child]
            pos = child
        d[pos] = elt
    return d


def reported_candidates(hits_of_read, as_score, got_pairs):
    """Where several hits tie with the reported score any of them may be the reported one (which one has a coordinate takes the index): the hit indices k, tied
    with as_score, for which the pairs are exactly the expectation over the hits in front of k in sorted_order.  A read passes if there is one.  For the top of the
    order that expectation is all the read's other hits."""
    h = np.asarray(hits_of_read)
    bits = h["score"].astype(np.float32).view(np.uint32)
    d = sorted_order(h["score"])
    got = _pair_key(got_pairs)
    return [d[j] for j in range(len(d) - 1, -1, -1) if bits[d[j]] == np.float32(as_score).view(np.uint32) and expected_pairs(h, d[j], d[:j]) == got]


def pairs_match(hits_of_read, as_score, got_pairs):
    return len(reported_candidates(hits_of_read, as_score, got_pairs)) > 0


def hits_by_read(res):
    hb = res.hit_begin.astype(np.int64)
    return [res.hits_arr[hb[i]:hb[i + 1]] for i in range(res.n_reads)]


def check_payload_against_hits(res, offsets, recs, extras):
    """Every mapped read of a decoded payload against the hit list it was made from: the pairs; best_size — the reported hit's size less the rows that have no
    coordinate inside a contig (mapping.rs:430-431), which is the record's X0: float32(x0), at most the hit's size and, but for reads at a contig's end, equal to
    it —; read_len, the read's length.  An unmapped read has no pairs, 0 and 0.  -> (mapped reads checked, those whose best_size is the hit's size)"""
    lens = np.diff(np.asarray(offsets).astype(np.int64))
    checked = whole = 0
    for i, h in enumerate(hits_by_read(res)):
        if not recs["mapped"][i]:
            assert len(extras["pairs"][i]) == 0 and extras["best_size"][i] == 0 and extras["read_len"][i] == 0, i
            continue
        cand = reported_candidates(h, recs["as_score"][i], extras["pairs"][i])
        assert cand, f"read {i}: pairs {extras['pairs'][i].tolist()} of hits {h.tolist()}"
        assert 0 < recs["x0"][i] < 0x7FFFFFFF and extras["best_size"][i].view(np.uint32) == np.float32(recs["x0"][i]).view(np.uint32), i
        sizes = h["size"][cand]
        assert (sizes >= recs["x0"][i]).any(), i
        whole += int((sizes == recs["x0"][i]).any())
        assert extras["read_len"][i] == lens[i], i
        checked += 1
    return checked, whole


def sub_batch(batch, lo, hi):
    seqs, quals, offsets = batch
    a, b = int(offsets[lo]), int(offsets[hi])
    return seqs[a:b], quals[a:b], (offsets[lo:hi + 1] - offsets[lo]).astype(np.uint64)


def shard_cuts(mapped):
    """Contiguous shards of a batch for the merge tests -> [(lo, hi)]: the reads in front of the batch's longest run of unmapped reads in two shards (a third and
    the rest: reads whose coordinate is drawn under the seed must lie in a shard that does not start at read 0), an EMPTY shard, that run — a shard in which no
    read mapped —, and what follows it (nothing, if the run ends the batch)."""
    m = np.concatenate([[True], np.asarray(mapped, bool), [True]])
    edges = np.flatnonzero(m)
    k = int(np.argmax(np.diff(edges)))
    lo, hi = int(edges[k]), int(edges[k + 1]) - 1  # reads [lo, hi) are unmapped
    cuts = [(0, lo // 3), (lo // 3, lo), (lo, lo), (lo, hi)]
    if hi < len(mapped):
        cuts.append((hi, len(mapped)))
    return cuts


def as_gather_parts(arrays):
    """(records int32 words, text bytes, pairs) of one shard as the three int32 CPU tensors a rank sends: the text padded to whole words"""
    import torch
    r, t, p = arrays
    t = np.ascontiguousarray(np.asarray(t)).view(np.uint8)
    t = np.concatenate([t, np.zeros(-len(t) % 4, np.uint8)])
    return tuple(torch.from_numpy(np.ascontiguousarray(x).view(np.int32).reshape(-1).copy()) for x in (np.asarray(r, np.int32), t, np.asarray(p).view(np.uint32)))


def repeat_batch(world, clean, n):
    """n 50-base reads from the five tandem copies of world A's repeat contig: nearly every read has XA entries, each with the contig's 48-character name"""
    from mapad_amd import synth
    rep0 = int(world.starts[1])
    return synth.reads(clean[rep0:rep0 + 3_000], n, 50, seed=411, qual_range=(20, 40), exo_frac=0.0)


REPEAT_READS = 1600  # about 150 bytes of record text per read against a first pool of 24 bytes per read + 64 KiB: tests/test_device_io_host.py holds the margin
