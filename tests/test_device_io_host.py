"""The host side of the device-resident calls' tests, without a GPU: tests/device_util.py's decoder of the gather payload is the exact inverse of an encoder written
here from the word layout of mapad_amd/distributed.py; merge_gathered_records over shards of world A (tests/records_util.py) — one of them empty, one without a
mapped read — gives the records of the whole batch and the oracle's; expected_pairs on hand-made hit lists; and the batch the GPU test overflows the per-slot text
pool with is sized here, from the host path's text lengths.  tests/test_gpu_device_io.py runs the same decoder, shards and batch over what mapad_records_device
returns."""
import numpy as np
import pytest

import mapad_amd
from mapad_amd import binding as mb
from mapad_amd.distributed import RECORD_WORDS, merge_gathered_records

import device_util as du
import emu_util
import records_util as ru
from parity_util import canonical_records, compare_records

PRESET = "damage"


def host_payload_inputs(res, recs, offsets):
    """what a payload carries beyond the record fields, from the hit lists: per read its pairs (the expectation of the last hit of device_util.sorted_order that is
    tied with the reported score, over the hits in front of it), float32(X0) and the read's length; nothing for an unmapped read"""
    lens = np.diff(np.asarray(offsets).astype(np.int64))
    pairs, best_size, read_len = [], np.zeros(len(recs), np.float32), np.zeros(len(recs), np.uint32)
    for i, h in enumerate(du.hits_by_read(res)):
        if not recs["mapped"][i]:
            pairs.append(np.zeros((0, 2), np.uint32))
            continue
        d = du.sorted_order(h["score"])
        j = max(j for j in range(len(d)) if h["score"][d[j]].view(np.uint32) == recs["as_score"][i].view(np.uint32))
        pairs.append(np.array(du.expected_pairs(h, d[j], d[:j]), np.uint32).reshape(-1, 2))
        best_size[i] = np.float32(recs["x0"][i])
        read_len[i] = lens[i]
    return pairs, best_size, read_len


def encode_device_records(recs, text, pairs, best_size, read_len, order):
    """mapad_record_t arrays -> (DevRecord words int32[n, 22], text pool uint8, pair pool uint32[k, 2]); the two pools are filled in the read order `order`, as
    the atomic claims of text_kernel's wavefronts fill them in whatever order they arrive"""
    n = len(recs)
    w = np.zeros((n, RECORD_WORDS), np.int32)
    u = w.view(np.uint32)
    t = np.asarray(text, np.uint8)
    pool, ppool = [], []
    n_text = n_pairs = 0
    for i in order:
        r = recs[i]
        if not r["mapped"]:
            w[i, 0:2] = -1
            w[i, 2] = -1
            continue
        w[i, 0:2] = np.array([r["pos"]], np.int64).view(np.int32)
        w[i, 2], u[i, 3], u[i, 4] = r["tid"], 1, r["reverse"]
        u[i, 5], u[i, 6] = np.float32(r["as_score"]).view(np.uint32), np.float32(r["xs_score"]).view(np.uint32)
        w[i, 7], w[i, 8], w[i, 9] = r["nm"], r["x0"], r["x1"]
        u[i, 10], u[i, 11] = r["has_xs"], r["xt"][0] if len(r["xt"]) else 0
        u[i, 12], u[i, 13], u[i, 14], u[i, 15] = n_text, r["cigar_len"], r["md_len"], r["xa_len"]
        for off, ln in ((r["cigar_off"], r["cigar_len"]), (r["md_off"], r["md_len"]), (r["xa_off"], r["xa_len"])):
            pool.append(t[int(off):int(off) + int(ln)])
            n_text += int(ln)
        u[i, 16], u[i, 17] = np.float32(best_size[i]).view(np.uint32), read_len[i]
        u[i, 18], u[i, 19] = n_pairs, len(pairs[i])
        ppool.append(np.asarray(pairs[i], np.uint32).reshape(-1, 2))
        n_pairs += len(pairs[i])
    return w, (np.concatenate(pool) if pool else np.zeros(0, np.uint8)), (np.concatenate(ppool) if ppool else np.zeros((0, 2), np.uint32))


def without_flags(recs):
    out = recs.copy()
    out["flags"] = 0
    out["mapq"] = 0
    return out


def same_records(got, want):
    """(records, text) pairs, compared field by field and text byte by text byte, wherever each side keeps a read's text"""
    return compare_records(canonical_records(*got, oracle_side=False), canonical_records(*want, oracle_side=False))


@pytest.fixture(scope="module")
def a():
    world, clean = ru.world_a()
    batch, straddlers = ru.reads_a(world, clean)
    p = ru.params(PRESET)
    res = emu_util.map_batch(world.pidx, p, *batch)
    recs, text = mapad_amd.hits_to_records(world.pidx, p, res, *batch, seed=ru.SEED, as_arrays=True)
    return dict(world=world, clean=clean, batch=batch, straddlers=straddlers, res=res, recs=recs, text=text, extra=host_payload_inputs(res, recs, batch[2]))


def test_decode_is_the_exact_inverse_of_the_word_layout(a):
    recs, text, (pairs, best_size, read_len) = a["recs"], a["text"], a["extra"]
    order = np.random.default_rng(5).permutation(len(recs))
    w, pool, ppool = encode_device_records(recs, text, pairs, best_size, read_len, order)
    assert int((w.view(np.uint32)[:, 12] > 0).sum()) > 1000 and not np.array_equal(np.argsort(w.view(np.uint32)[:, 12], kind="stable"), np.arange(len(recs)))  # the pool is not in read order
    got, gtext, extras = du.decode_device_records(w.reshape(-1), pool, ppool.view(np.float32).reshape(-1))
    n_bad, first, per_field = same_records((got, gtext), (without_flags(recs), text))
    assert n_bad == 0, ru.report(first, per_field)
    m = recs["mapped"] != 0
    for k in ("pos", "tid", "mapped"):  # of every read, mapped or not
        assert np.array_equal(got[k], recs[k]), k
    for k in ("reverse", "nm", "x0", "x1", "has_xs", "xt", "cigar_len", "md_len", "xa_len"):
        assert np.array_equal(got[k][m], recs[k][m]), k
    assert np.array_equal(got["as_score"][m].view(np.uint32), recs["as_score"][m].view(np.uint32)) and not got["flags"].any() and not got["mapq"].any()
    assert all(np.array_equal(x, y) for x, y in zip(extras["pairs"], pairs)) and sum(len(x) for x in pairs) > 100
    assert np.array_equal(extras["best_size"].view(np.uint32), best_size.view(np.uint32)) and np.array_equal(extras["read_len"], read_len) and not extras["error"].any()
    checked, whole = du.check_payload_against_hits(a["res"], a["batch"][2], got, extras)
    assert checked == int(m.sum()) and checked - 20 <= whole < checked  # (a few reads at a contig's end: X0 is less than the rows of their hit)
    # and the other way round: what the decoder returns encodes to the same words
    w2, pool2, ppool2 = encode_device_records(got, gtext, extras["pairs"], extras["best_size"], extras["read_len"], order)
    assert np.array_equal(w2, w) and np.array_equal(pool2, pool) and np.array_equal(ppool2, ppool)


def test_merged_shards_equal_the_whole_batch_and_the_oracle(a):
    """Contiguous shards, among them an empty one and one in which no read mapped (device_util.shard_cuts: the longest unmapped run of world A lies inside the
    batch, so a last shard holds what follows it; the reads in front of it make two shards), each with pools in an order of its own, through merge_gathered_records as CPU tensors."""
    recs, text, (pairs, best_size, read_len) = a["recs"], a["text"], a["extra"]
    n = len(recs)
    cuts = du.shard_cuts(recs["mapped"] != 0)
    assert cuts[2][0] == cuts[2][1] and cuts[3][1] - cuts[3][0] >= 64 and not recs["mapped"][cuts[3][0]:cuts[3][1]].any() and cuts[-1][1] == n, cuts
    assert int((recs["x0"][cuts[1][0]:cuts[1][1]] >= 3).sum()) >= 100  # reads whose coordinate is drawn under the seed, in a shard that starts behind read 0
    parts = []
    for k, (lo, hi) in enumerate(cuts):
        order = np.random.default_rng(10 + k).permutation(hi - lo)
        parts.append(du.as_gather_parts(encode_device_records(recs[lo:hi], text, pairs[lo:hi], best_size[lo:hi], read_len[lo:hi], order)))
    assert parts[2][0].numel() == 0 and parts[3][1].numel() == 0 and parts[3][2].numel() == 0
    m_recs, m_text, m_pairs, _ = merge_gathered_records(parts)
    got, gtext, extras = du.decode_device_records(m_recs, m_text, m_pairs)
    whole = du.decode_device_records(*encode_device_records(recs, text, pairs, best_size, read_len, np.arange(n)))
    n_bad, first, per_field = same_records((got, gtext), whole[:2])
    assert n_bad == 0, ru.report(first, per_field)
    assert all(np.array_equal(x, y) for x, y in zip(extras["pairs"], whole[2]["pairs"]))
    assert np.array_equal(extras["best_size"], whole[2]["best_size"]) and np.array_equal(extras["read_len"], whole[2]["read_len"])
    ocanon = du.without_flags_and_mapq(a["world"].oracle_canon(PRESET, a["res"], a["batch"]))
    n_bad, first, per_field = ru.differing((got, gtext), ocanon)
    assert n_bad == 0, ru.report(first, per_field)
    ru.check_reach_a(ru.edge_counts_a(a["world"], got, gtext, a["straddlers"], a["res"].hit_begin))


def _hits(rows):
    h = np.zeros(len(rows), mb.HIT_DTYPE)
    for k, (lower, lower_rev, size, score) in enumerate(rows):
        h[k] = (lower, lower_rev, size, score, 50, 0, 0)
    return h


def _bits(score, size):
    return (int(np.float32(score).view(np.uint32)), int(np.float32(size).view(np.uint32)))


def test_expected_pairs_on_hand_made_hit_lists():
    # a tie at the top: either of the two may be the reported hit, and then the other one counts
    tie = _hits([(10, 100, 1, -1.0), (20, 200, 1, -1.0), (30, 300, 2, -3.5)])
    assert du.expected_pairs(tie, 0) == sorted([_bits(-1.0, 1), _bits(-3.5, 2)]) == du.expected_pairs(tie, 1)
    assert du.pairs_match(tie, np.float32(-1.0), np.array([_bits(-3.5, 2), _bits(-1.0, 1)], np.uint32))  # in any order
    assert du.sorted_order(tie["score"])[0] == 2 and sorted(du.sorted_order(tie["score"])[1:]) == [0, 1]
    assert du.pairs_match(tie, np.float32(-1.0), np.array([_bits(-3.5, 2)], np.uint32))  # the first of the two had no coordinate and was dropped: the second is reported
    assert not du.pairs_match(tie, np.float32(-1.0), np.array([_bits(-1.0, 1)], np.uint32)) and not du.pairs_match(tie, np.float32(-1.0), np.zeros((0, 2), np.uint32))
    assert not du.pairs_match(tie, np.float32(-3.5), np.array([_bits(-1.0, 1)], np.uint32)) and du.pairs_match(tie, np.float32(-3.5), np.zeros((0, 2), np.uint32))
    assert not du.pairs_match(tie, np.float32(-1.0), np.array([_bits(-3.5, 2), _bits(-1.0, 1), _bits(-1.0, 1)], np.uint32))  # a multiset, not a set
    tie2 = _hits([(10, 100, 1, -1.0), (20, 200, 3, -1.0), (30, 300, 2, -3.5)])  # tied scores, different sizes: two different expectations
    assert du.expected_pairs(tie2, 0) != du.expected_pairs(tie2, 1)
    top = du.sorted_order(tie2["score"])[-1]
    assert du.reported_candidates(tie2, np.float32(-1.0), np.array(du.expected_pairs(tie2, top), np.uint32)) == [top]
    assert not du.pairs_match(tie2, np.float32(-1.0), np.array(du.expected_pairs(tie2, 1 - top), np.uint32))  # the other one is reported only once the top is dropped
    assert du.pairs_match(tie2, np.float32(-1.0), np.array([_bits(-3.5, 2)], np.uint32))
    rng = np.random.default_rng(3)  # over a heap array (a descending one is a heap) the order is a sorted one
    for n in (1, 2, 3, 7, 20):
        sc = np.sort(-rng.integers(0, 4, n).astype(np.float32))[::-1].copy()
        assert (np.diff(sc[du.sorted_order(sc)]) >= 0).all() and sorted(du.sorted_order(sc)) == list(range(n))
    # cross-matching hits: the same size and the same lower, or the same lower_rev, as the reported one do not count; another size does
    cross = _hits([(10, 50, 2, -0.5), (10, 70, 2, -2.0), (11, 50, 2, -2.5), (10, 50, 3, -3.0), (12, 52, 2, -4.0)])
    assert du.expected_pairs(cross, 0) == sorted([_bits(-3.0, 3), _bits(-4.0, 2)])
    assert du.expected_pairs(cross, 4) == sorted([_bits(-0.5, 2), _bits(-2.0, 2), _bits(-2.5, 2), _bits(-3.0, 3)])
    assert ru.pairs_needed(ru.CallerResult.from_lists([cross], np.zeros(64, np.uint32)), np.array([(1, -0.5)], [("mapped", "u1"), ("as_score", "<f4")])) == 2
    # a single hit: no pairs
    one = _hits([(10, 50, 7, -1.25)])
    assert du.expected_pairs(one, 0) == [] and du.pairs_match(one, np.float32(-1.25), np.zeros((0, 2), np.uint32))
    assert not du.pairs_match(one, np.float32(-1.25), np.array([_bits(-1.25, 7)], np.uint32))


def test_the_repeat_batch_outgrows_the_first_text_pool(a):
    """What test_gpu_device_io.py's overflow case needs of its batch: its record text is more than twice what run_record_kernels asks for on first use (the factor
    covers the slack of the allocation, records_util.initial_pools).  The pair pool cannot be overrun in this world: reads on (ACGTTGCA) x 500 leave a quarter of a
    pair each, and the pool starts at n + 2048."""
    world, clean = a["world"], a["clean"]
    batch = du.repeat_batch(world, clean, du.REPEAT_READS)
    p = ru.params(PRESET)
    res = emu_util.map_batch(world.pidx, p, *batch)
    recs, rtext = mapad_amd.hits_to_records(world.pidx, p, res, *batch, seed=ru.SEED, as_arrays=True)
    text_bytes = int(recs["cigar_len"].sum() + recs["md_len"].sum() + recs["xa_len"].sum())
    print("repeat batch:", du.REPEAT_READS, "reads,", text_bytes, "text bytes, first pool", ru.initial_pools(du.REPEAT_READS))
    assert text_bytes > 2 * ru.initial_pools(du.REPEAT_READS)[0]
    xa = [rtext[int(r["xa_off"]):int(r["xa_off"]) + int(r["xa_len"])].tobytes() for r in recs]
    assert sum(ru.A_REP_NAME.encode() in x for x in xa) >= du.REPEAT_READS // 2  # the 48-character name in the XA entries is what makes the text long
