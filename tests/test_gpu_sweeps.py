"""GPU parity sweeps (run with -m gpu on an MI355X): the cases of tests/sweep_util.py — search parameters the presets never vary, read lengths around every
threshold at which a launch changes its memory layout, a reference with repeats, an X run and contig joins — through the HIP path, every word of every result
against the CPU oracle.  tests/test_sweeps_host.py runs the same tables through the host build of the per-read logic."""
import pytest

import mapad_amd

import sweep_util as su
from parity_util import assert_same_as_oracle, rerun_in_heavy_build

pytestmark = pytest.mark.gpu


world = pytest.fixture(scope="module")(su.grid_world)
struct_worlds = pytest.fixture(scope="module")(su.struct_worlds)


def _gpu_map(world, rp, batch):
    ctx = mapad_amd.Context(world.pidx, mapad_amd.make_params(rp), 0)  # (the launch switches of the environment are read here)
    try:
        return ctx.map_batch(*batch)
    finally:
        ctx.close()


def _env_id(cid, env):
    return cid + "-" + ",".join(f"{k[6:].lower()}={v}" for k, v in env.items()) if env else cid


# ---- A. parameter grid ----------------------------------------------------------------------------------------------------------------------------------------
_GRID = [(cid, {}) for cid in su.GRID_IDS] + su.GRID_LAUNCH_VARIANTS


@pytest.mark.parametrize("cid,env", _GRID, ids=[_env_id(*c) for c in _GRID])
def test_parameter_grid(world, cid, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rp, _ = su.grid_case(cid)
    ores = world.oracle(("grid", cid), rp, world.grid_batch)
    su.check_grid_reach(cid, ores)
    assert_same_as_oracle(ores, _gpu_map(world, rp, world.grid_batch), world.grid_batch[2])


# ---- B. length ladders ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes_per_read", ["4", "2", "1"])
@pytest.mark.parametrize("mid", su.B1_IDS)
def test_every_length_from_1_to_130(world, mid, lanes_per_read, monkeypatch):
    monkeypatch.setenv("MAPAD_LANES_PER_READ", lanes_per_read)
    rp = su.b1_params(mid)
    batch = su.ladder_reads(world.genome, su.B1_LENGTHS, seed=su.B1_SEED)
    ores = world.oracle(("b1", mid), rp, batch)
    su.check_ladder_reach(ores, batch[2])
    assert_same_as_oracle(ores, _gpu_map(world, rp, batch), batch[2])


@pytest.mark.parametrize("lanes_per_read", ["4", "2", "1"])
@pytest.mark.parametrize("mid", su.B1_IDS)
def test_batch_of_reads_shorter_than_the_offset_chains(world, mid, lanes_per_read, monkeypatch):
    monkeypatch.setenv("MAPAD_LANES_PER_READ", lanes_per_read)
    rp = su.b1_params(mid)
    batch = su.ladder_reads(world.genome, su.B1_SHORT_ONLY, seed=su.B1_SEED)
    ores = world.oracle(("b1_short", mid), rp, batch)
    assert su.hits_per_read(ores).astype(bool).sum() >= 2  # the longest of them map
    assert_same_as_oracle(ores, _gpu_map(world, rp, batch), batch[2])


# (lmax, lanes per read, heavy build): see the table of thresholds in sweep_util.py
_LAYOUT = ([(lmax, "1", False) for lmax in su.B1_SINGLE_LANE_LMAX] + [(lmax, "4", False) for lmax in su.B2_LMAX] + [(lmax, "2", False) for lmax in su.B2_PAIRS_LMAX]
           + [(lmax, "4", True) for lmax in su.B2_HEAVY_LMAX])


@pytest.mark.parametrize("lmax,lanes_per_read,heavy", _LAYOUT, ids=[f"{lmax}-lanes{lpr}" + ("-heavy" if heavy else "") for lmax, lpr, heavy in _LAYOUT])
def test_layout_threshold_lengths(lmax, lanes_per_read, heavy, monkeypatch, request):
    if heavy:
        if rerun_in_heavy_build(request):  # (before the world is built: the parent only starts the child)
            return
        monkeypatch.setenv("MAPAD_HEAVY", "1")
        monkeypatch.setenv("MAPAD_TIER0_NODES", "64")  # small base arenas: the reads are suspended by their quads and finished by a wavefront of their own
    monkeypatch.setenv("MAPAD_LANES_PER_READ", lanes_per_read)
    world = request.getfixturevalue("world")
    rp = su.b1_params("damage")
    batch = su.layout_batch(world.genome, lmax)
    ores = world.oracle(("b2", lmax), rp, batch)
    su.check_ladder_reach(ores, batch[2])
    res = _gpu_map(world, rp, batch)
    if heavy:
        assert res.n_second_pass > 0  # reads really were suspended
    assert_same_as_oracle(ores, res, batch[2])


# ---- C. structured reference ----------------------------------------------------------------------------------------------------------------------------------
_STRUCT = [(cid, {}) for cid in su.STRUCT_IDS] + su.STRUCT_LAUNCH_VARIANTS


@pytest.mark.parametrize("cid,env", _STRUCT, ids=[_env_id(*c) for c in _STRUCT])
def test_structured_reference(struct_worlds, cid, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    w, rp, batch = su.struct_case(cid, struct_worlds)
    ores = w.oracle(("struct", cid), rp, batch)
    su.check_struct_reach(cid, w, struct_worlds[False][2], ores)
    if "MAPAD_HIT_POOL" in env:
        assert int(ores.hit_offsets[-1]) > int(env["MAPAD_HIT_POOL"])  # the pool overflows: the launch is retried
    res = _gpu_map(w, rp, batch)
    if "MAPAD_TIER0_NODES" in env:
        assert res.n_second_pass > 0  # reads outgrew their base arenas
    assert_same_as_oracle(ores, res, batch[2])


def test_edit_tree_of_six_million_nodes(world):
    """Gaps at -4 / -1 with the reference's own limits: one read of 2.9 M pops and 6.0 M edit-tree nodes (sweep_util.EXPLOSIVE_GAP; the CPU side and the story of
    the read are in tests/test_sweeps_host.py).  On the GPU such a read leaves its quad for the full-limit stage and the host tail."""
    rp, batch = su.explosive_case(world)
    ores = world.oracle("explosive", rp, batch)
    su.check_explosive_reach(ores)
    assert_same_as_oracle(ores, _gpu_map(world, rp, batch), batch[2])
