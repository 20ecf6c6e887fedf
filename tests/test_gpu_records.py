"""GPU tests of the post-search record kernels — records_kernel (postproc_core.hpp: into_sorted_vec, PrRange, the suffix-array walk, strand and contig, X0 / X1, the
XA candidates) and text_kernel (text_core.hpp: CIGAR / MD / NM / XA text, the pairs of the mapping quality, the pools and their overflow rerun in
run_record_kernels) — against the independent oracle's intervals_to_record, on the small worlds of tests/records_util.py (tests/test_records_host.py is the CPU
twin over the same table).  Every field of every record must be equal."""
import pytest

import mapad_amd

import records_util as ru
from parity_util import canonical_records, check_ungapped_records_against_the_text, compare_records, records_digest

pytestmark = pytest.mark.gpu

TEXT_MODES = ["device", "host"]  # MAPAD_RECORDS_TEXT: CIGAR / MD / XA and the MAPQ's pairs by text_kernel | strings on host threads from records_kernel's coordinates


@pytest.fixture(scope="module")
def a():
    """world A, its reads, and per preset (lazily): an open context with the batch's result still resident on the device, and the oracle's records over its hits"""
    world, clean = ru.world_a()
    batch, straddlers = ru.reads_a(world, clean)
    mapped = {}

    def run(preset):
        if preset not in mapped:
            ctx = mapad_amd.Context(world.pidx, ru.params(preset), 0)
            res = ctx.map_batch(*batch)
            mapped[preset] = (ctx, res, world.oracle_canon(preset, res, batch))
        return mapped[preset]

    yield world, clean, batch, straddlers, run
    for ctx, _, _ in mapped.values():
        ctx.close()


@pytest.fixture(scope="module")
def b():
    """world B: the caller-built hit lists over what the GPU search finds, the wavefront-edge batches made of them, and the oracle's records of each"""
    world, text, starts = ru.world_b()
    batch = ru.reads_b(text, starts)
    ctx = mapad_amd.Context(world.pidx, ru.params(ru.B_PRESET), 0)
    try:
        cres = ru.hit_lists_b(ctx.map_batch(*batch))
    finally:
        ctx.close()
    cases = dict(ru.edge_batches_b(cres), lists=cres)
    return world, batch, cases, {k: world.oracle_canon(ru.B_PRESET, c, batch) for k, c in cases.items()}


def _fresh(world, preset):
    return mapad_amd.Context(world.pidx, ru.params(preset), 0)


def _head(batch, k):
    seqs, quals, offsets = batch
    return seqs[:int(offsets[k])], quals[:int(offsets[k])], offsets[:k + 1]


@pytest.mark.parametrize("preset", list(ru.PRESETS))
@pytest.mark.parametrize("text", TEXT_MODES)
def test_world_a_records_equal_the_oracles(a, text, preset, monkeypatch):
    monkeypatch.setenv("MAPAD_RECORDS_TEXT", text)
    world, clean, batch, straddlers, run = a
    ctx, res, ocanon = run(preset)
    recs, rtext = ctx.hits_to_records(res, *batch, seed=ru.SEED, as_arrays=True)
    n_bad, first, per_field = ru.differing((recs, rtext), ocanon)
    counts = ru.edge_counts_a(world, recs, rtext, straddlers, res.hit_begin)
    print(text, preset, counts)
    assert n_bad == 0, ru.report(first, per_field)
    ru.check_reach_a(counts)
    checked, failed = check_ungapped_records_against_the_text(clean, ru.ungapped_text_check_input(world, recs, batch[2]), rtext, batch[0], batch[2], contig_starts=world.starts[:-1])
    assert checked > 1000 and failed == 0


@pytest.mark.parametrize("text", TEXT_MODES)
def test_world_b_caller_built_hit_lists_equal_the_oracles(b, text, monkeypatch):
    """the uploaded path: the result has no private half, its hits go to the device first"""
    monkeypatch.setenv("MAPAD_RECORDS_TEXT", text)
    world, batch, cases, ocanon = b
    ctx = _fresh(world, ru.B_PRESET)
    try:
        recs, rtext = ctx.hits_to_records(cases["lists"], *batch, seed=ru.SEED, as_arrays=True)
    finally:
        ctx.close()
    n_bad, first, per_field = ru.differing((recs, rtext), ocanon["lists"])
    assert n_bad == 0, ru.report(first, per_field)
    ru.check_reach_b(ru.edge_counts_b(cases["lists"], recs))


def test_pool_overflow_rerun(b, monkeypatch):
    """World B as the first conversion of a fresh context (the pools only ever grow within one): its record text and its pairs are more than twice what
    run_record_kernels starts with, so text_kernel runs, overflows both pools, and runs again in grown ones.  Then a small batch in the grown pools."""
    monkeypatch.setenv("MAPAD_RECORDS_TEXT", "device")
    world, batch, cases, ocanon = b
    cres = cases["lists"]
    text_cap, pair_cap = ru.initial_pools(cres.n_reads)  # mapad_amd.hip: run_record_kernels: text.ensure(n * 24 + (1 << 16)), pairs.ensure(n * 2 + 4096) floats
    ctx = _fresh(world, ru.B_PRESET)
    try:
        recs, rtext = ctx.hits_to_records(cres, *batch, seed=ru.SEED, as_arrays=True)
        small = ctx.hits_to_records(cres.prefix(65), *_head(batch, 65), seed=ru.SEED, as_arrays=True)
    finally:
        ctx.close()
    text_bytes = int(recs["cigar_len"].sum() + recs["md_len"].sum() + recs["xa_len"].sum())
    pairs = ru.pairs_needed(cres, recs)
    print(f"text bytes {text_bytes} (pool {text_cap}), pairs >= {pairs} (pool {pair_cap})")
    assert len(rtext) == text_bytes > 2 * text_cap and pairs > 2 * pair_cap
    n_bad, first, per_field = ru.differing((recs, rtext), ocanon["lists"])
    assert n_bad == 0, ru.report(first, per_field)
    n_bad, first, per_field = ru.differing(small, ocanon["lists"], 0, 65)
    assert n_bad == 0, ru.report(first, per_field)


@pytest.mark.parametrize("text", TEXT_MODES)
def test_partial_wavefronts(b, text, monkeypatch):
    """the first 1, 63, 64, 65 and 129 reads of the caller-built result: a lane, a wavefront less one, a full one, one more, two and one"""
    monkeypatch.setenv("MAPAD_RECORDS_TEXT", text)
    world, batch, cases, ocanon = b
    ctx = _fresh(world, ru.B_PRESET)
    try:
        for k in ru.PREFIXES_B:
            got = ctx.hits_to_records(cases["lists"].prefix(k), *_head(batch, k), seed=ru.SEED, as_arrays=True)
            n_bad, first, per_field = ru.differing(got, ocanon["lists"], 0, k)
            assert n_bad == 0 and (got[0]["mapped"] != 0).all(), ru.report(first, per_field, k)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", ["first_64_without_hits", "all_unmapped", "no_second_hit"])
def test_unmapped_wavefronts_and_batches_without_pairs(b, case, monkeypatch):
    world, batch, cases, ocanon = b
    for text in TEXT_MODES:
        monkeypatch.setenv("MAPAD_RECORDS_TEXT", text)
        ctx = _fresh(world, ru.B_PRESET)
        try:
            recs, rtext = ctx.hits_to_records(cases[case], *batch, seed=ru.SEED, as_arrays=True)
        finally:
            ctx.close()
        n_bad, first, per_field = ru.differing((recs, rtext), ocanon[case])
        assert n_bad == 0, ru.report(first, per_field, text)
        m = recs["mapped"] != 0
        if case == "first_64_without_hits":
            assert not m[:64].any() and m[64:].all() and (recs["flags"][:64] & 0x4).all() and (recs["tid"][:64] == -1).all() and (recs["pos"][:64] == -1).all()
        elif case == "all_unmapped":
            assert not m.any() and len(rtext) == 0 and (recs["flags"] & 0x4).all() and (recs["mapq"] == 0).all()
        else:
            assert m.all() and ru.pairs_needed(cases[case], recs) == 0 and not recs["has_xs"].any()


@pytest.mark.parametrize("text", TEXT_MODES)
def test_resident_and_uploaded_hits_give_the_same_records(a, text, monkeypatch):
    """the context's own result (its hits still on the device, where the launch left them) and a caller-built copy of the same arrays (uploaded)"""
    monkeypatch.setenv("MAPAD_RECORDS_TEXT", text)
    world, clean, batch, straddlers, run = a
    ctx, res, ocanon = run("damage")
    own = canonical_records(*ctx.hits_to_records(res, *batch, seed=ru.SEED, as_arrays=True)[:2], oracle_side=False)
    uploaded = canonical_records(*ctx.hits_to_records(ru.copy_of(res), *batch, seed=ru.SEED, as_arrays=True)[:2], oracle_side=False)
    n_bad, first, per_field = compare_records(own, uploaded)
    assert n_bad == 0 and records_digest(own) == records_digest(uploaded), ru.report(first, per_field)
    again = canonical_records(*ctx.hits_to_records(res, *batch, seed=ru.SEED, as_arrays=True)[:2], oracle_side=False)  # the upload left the resident result alone
    assert records_digest(again) == records_digest(own)
    assert compare_records(own, ocanon)[0] == 0
    # the same result sent the long way (MAPAD_RECORDS_RESIDENT=0: its hits are uploaded like a caller's)
    monkeypatch.setenv("MAPAD_RECORDS_RESIDENT", "0")
    forced = canonical_records(*ctx.hits_to_records(res, *batch, seed=ru.SEED, as_arrays=True)[:2], oracle_side=False)
    monkeypatch.delenv("MAPAD_RECORDS_RESIDENT")
    assert records_digest(forced) == records_digest(own)
    # ... and which branch ran, observed: with the damage profile on, record_coords_gpu refuses hits it has to upload (their reads are no longer on the device)
    ctx.set_damage_profile(1)
    try:
        ctx.hits_to_records(res, *batch, seed=ru.SEED, as_arrays=True)  # resident: accepted
        with pytest.raises(mapad_amd.MapadError):
            ctx.hits_to_records(ru.copy_of(res), *batch, seed=ru.SEED, as_arrays=True)
        monkeypatch.setenv("MAPAD_RECORDS_RESIDENT", "0")
        with pytest.raises(mapad_amd.MapadError):
            ctx.hits_to_records(res, *batch, seed=ru.SEED, as_arrays=True)
    finally:
        monkeypatch.delenv("MAPAD_RECORDS_RESIDENT", raising=False)
        ctx.set_damage_profile(0)
