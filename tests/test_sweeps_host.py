"""CPU twin of tests/test_gpu_sweeps.py: the cases of tests/sweep_util.py through the host build of the kernels' per-read logic (emu_util.map_batch) against the
oracle.  It validates the case tables and their reach-conditions without a GPU and protects the step code the kernels share (csrc/search_core.hpp,
csrc/darray_core.hpp).  What only changes a launch — lanes per read, the heavy build, the hit pool — has no counterpart here."""
import numpy as np
import pytest

import mapad_amd

import emu_util
import sweep_util as su
from parity_util import assert_same_as_oracle


world = pytest.fixture(scope="module")(su.grid_world)
struct_worlds = pytest.fixture(scope="module")(su.struct_worlds)


def _emu(world, rp, batch, **caps):
    return emu_util.map_batch(world.pidx, mapad_amd.make_params(rp), *batch, **caps)


@pytest.mark.parametrize("cid", su.GRID_IDS)
def test_parameter_grid(world, cid):
    rp, _ = su.grid_case(cid)
    ores = world.oracle(("grid", cid), rp, world.grid_batch)
    su.check_grid_reach(cid, ores)
    assert_same_as_oracle(ores, _emu(world, rp, world.grid_batch), world.grid_batch[2])


@pytest.mark.parametrize("mid", su.B1_IDS)
def test_every_length_from_1_to_130(world, mid):
    rp = su.b1_params(mid)
    batch = su.ladder_reads(world.genome, su.B1_LENGTHS, seed=su.B1_SEED)
    ores = world.oracle(("b1", mid), rp, batch)
    su.check_ladder_reach(ores, batch[2])
    assert_same_as_oracle(ores, _emu(world, rp, batch), batch[2])


@pytest.mark.parametrize("mid", su.B1_IDS)
def test_batch_of_reads_shorter_than_the_offset_chains(world, mid):
    rp = su.b1_params(mid)
    batch = su.ladder_reads(world.genome, su.B1_SHORT_ONLY, seed=su.B1_SEED)
    ores = world.oracle(("b1_short", mid), rp, batch)
    assert su.hits_per_read(ores).astype(bool).sum() >= 2  # the longest of them map
    assert_same_as_oracle(ores, _emu(world, rp, batch), batch[2])


@pytest.mark.parametrize("lmax", su.B1_SINGLE_LANE_LMAX + su.B2_LMAX)
def test_layout_threshold_lengths(world, lmax):
    rp = su.b1_params("damage")
    batch = su.layout_batch(world.genome, lmax)
    ores = world.oracle(("b2", lmax), rp, batch)
    su.check_ladder_reach(ores, batch[2])
    assert_same_as_oracle(ores, _emu(world, rp, batch), batch[2])


@pytest.mark.parametrize("cid", su.STRUCT_IDS)
def test_structured_reference(struct_worlds, cid):
    w, rp, batch = su.struct_case(cid, struct_worlds)
    ores = w.oracle(("struct", cid), rp, batch)
    su.check_struct_reach(cid, w, struct_worlds[False][2], ores)
    assert_same_as_oracle(ores, _emu(w, rp, batch), batch[2])
    if cid == "three_contigs_no_damage_q40":  # and with arenas of 32 nodes: migrations and full-limit re-runs
        res = _emu(w, rp, batch, node_cap=32, heap_cap=32)
        assert res.n_second_pass > 0
        assert_same_as_oracle(ores, res, batch[2])


def test_edit_tree_of_six_million_nodes(world):
    """Gaps at -4 / -1 with the reference's own limits: one read whose search takes 2.9 M pops and 6.0 M edit-tree nodes (sweep_util.EXPLOSIVE_GAP), through the
    per-read logic with node indices far past 2^22 and through the host tail's search (csrc/host_tail.hpp: tail_search), which is what finishes such a read in
    production.  With these settings the emulation used to disagree with the oracle ("hit counts differ") on exactly the reads of more than 2^22 nodes: emu.cpp
    capped the backing stores of its full-limit pass at 2^22 entries, below the 10 M limit, so those reads ended with an arena overflow.  The step, the frame and
    the node-index fields were never wrong; emu.cpp now repeats such a read in stores as large as the limits.  The slowest case of the file, about 12 s: the oracle's
    search, the emulation's passes 0, 1 (which overflows, by design of the case) and 2, and the host tail's search, 2.9 M pops each."""
    rp, batch = su.explosive_case(world)
    ores = world.oracle("explosive", rp, batch)
    su.check_explosive_reach(ores)
    res = _emu(world, rp, batch)
    assert res.status[0] == 0
    assert_same_as_oracle(ores, res, batch[2])
    _, pops, status, _, _ = emu_util.tail_search(world.pidx, mapad_amd.make_params(rp), *batch, np.arange(1), threads=1)
    assert int(pops[0]) == int(ores.counters[0, 3]) and int(status[0]) == 0
