"""broadphase::BVH on the device at edge leaf counts and degenerate layouts: the
plan mode of sims/broadphase_only (DESIGN.md "Broadphase plan mode") in lock
step with the reference backend, every step, bit for bit.

Leaf counts 0 .. 6, 8, 9, 16 .. 21, 31 .. 33, 60 .. 66, 96, 97, 128 .. 130, a small
tree next to a large one in every pair of adjacent worlds (the two halves of a
wavefront: different window counts in traceRayShared and in the 32-lane box
queries); layouts whose leaf centres tie on purpose (the reference's axis
choice with strict >, its swap partition, its n / 2 fallback and its empty
sub-ranges, which the breadth-first device build must reproduce exactly);
max_leaves at the leaf count, at 64 (staged build at its capacity limit) and at
65 (the same leaves built in place: staging depends on the node capacity).
test_bvh_edges_cpu.py pins the reference itself (float64 brute force) and shows
that every planned input stays inside the reference's unchecked node array and
stacks; the reference runs L = 0 and L = 1 cleanly, so they are in the lock step.
"""
import numpy as np
import pytest

import bvh_edges_utils as U
from madrona_amd.simlib import Simulator, hip_lib_path, ref_lib_path

pytestmark = pytest.mark.gpu

SIM = "broadphase_only"
WORLDS = 56         # two passes through the leaf table: every L in both halves
STEPS = 12          # rebuilds at steps 1, 4, 8, 12, from two input orders
SEED = 3

EXACT_COLUMNS = ("Box.Position", "Box.LeafID", "Pillar.LeafID", "Sensor.Position",
                 "Sensor.RayFan", "Sensor.RayFanPlain", "Prober.Probe32",
                 "Prober.Probe64")


def _lock_step(layout, mode, no_pillars=False, worlds=WORLDS):
    if not U.plan_mode_built(ref_lib_path(SIM)):
        pytest.skip(f"reference backend of {SIM} absent from oracle/_ref, or built "
                    "from sources without the plan mode")
    flags = U.plan_flags(layout, mode, no_pillars)
    table = U.LEAF_TABLE
    leaves = np.array([table[w % len(table)] for w in range(worlds)])
    ray_hits = np.zeros(worlds, np.int64)
    with Simulator(ref_lib_path(SIM), worlds, seed=SEED, num_workers=1,
                   flags=flags) as ref, \
            Simulator(hip_lib_path(SIM), worlds, seed=SEED, flags=flags) as hip:
        for step in range(1, STEPS + 1):
            ref.step(1)
            hip.step(1)         # (a device error flag fails the step)
            rd, hd = U.dump_plan(ref), U.dump_plan(hip)
            where = (layout, mode, no_pillars, worlds, step)

            for col in EXACT_COLUMNS:
                assert np.array_equal(rd[col][1], hd[col][1]), (where, col, "rows per world")
                if not np.array_equal(rd[col][0], hd[col][0]):
                    r_rows, h_rows = rd[col][0], hd[col][0]
                    bad = np.nonzero((r_rows != h_rows).any(axis=1))[0]
                    world_of_row = np.repeat(np.arange(worlds), rd[col][1])
                    w = int(world_of_row[bad[0]])
                    words = np.nonzero(r_rows[bad[0]].view(np.int32) !=
                                       h_rows[bad[0]].view(np.int32))[0]
                    pytest.fail(f"{where} {col}: {len(bad)} rows differ, first row "
                                f"{bad[0]} (world {w}, {leaves[w]} leaves), words "
                                f"{words[:8].tolist()}: reference "
                                f"{r_rows[bad[0]].view(np.int32)[words[:8]].tolist()} "
                                f"device {h_rows[bad[0]].view(np.int32)[words[:8]].tolist()}")

            # the candidate pairs in order (the order is the traversal order:
            # it pins the tree shape)
            r_counts = rd["Candidates.CandidateCollision"][1]
            h_counts = hd["Candidates.CandidateCollision"][1]
            assert np.array_equal(r_counts, h_counts), (where, "pairs per world")
            r_pairs = U.candidate_ids(rd, local_rows=True)
            h_pairs = U.candidate_ids(hd, local_rows=False)
            if not np.array_equal(r_pairs, h_pairs):
                bad = np.nonzero((r_pairs != h_pairs).any(axis=1))[0]
                pytest.fail(f"{where} candidate pairs: {len(bad)} differ, first "
                            f"(world, a, b) reference {r_pairs[bad[0]].tolist()} "
                            f"device {h_pairs[bad[0]].tolist()}")

            # ---- guards against a vacuous case ----
            bodies = rd["Box.LeafID"][1] + rd["Pillar.LeafID"][1]
            assert np.array_equal(bodies, leaves), where
            if no_pillars:
                assert rd["Pillar.LeafID"][1].sum() == 0
            sensors = rd["Sensor.RayFan"][1]
            fan = hd["Sensor.RayFan"][0].view(np.int32).reshape(-1, 160)
            ray_hits += np.add.reduceat(
                (fan[:, 32:64] >= 0).sum(axis=1),
                np.concatenate([[0], np.cumsum(sensors)[:-1]]))
            probes = (hd["Prober.Probe32"][0].view(np.int32).reshape(-1, 4),
                      hd["Prober.Probe64"][0].view(np.int32).reshape(-1, 4))
            boxes = rd["Box.LeafID"][1]
            for probe in probes:
                assert len(probe) == worlds
                assert np.all(probe[boxes > 0, 3] >= 0), where
                assert np.all(probe[leaves == 0] == -1), where
            if layout in ("coincident", "outlier", "nested"):
                # (outlier: all but one coincide)
                crowd = boxes >= (3 if layout == "outlier" else 2)
                assert np.all(h_counts[crowd] > 0), where
            assert np.all(h_counts[leaves <= 1] == 0), where
    assert set(leaves) == set(table)
    assert np.all(ray_hits[leaves > 0] > 0), (layout, mode, np.nonzero(ray_hits == 0)[0])
    assert np.all(ray_hits[leaves == 0] == 0)


@pytest.mark.parametrize("layout,mode", U.plan_cases())
def test_plan_lock_step(built, monkeypatch, layout, mode):
    """Every layout at every max_leaves mode.  max_leaves 64 against 65 on the
    same leaves is the boundary of rebuildTreeStaged's staging: node capacity
    85 (staged, at the limit of the LDS node array) against 87 (lane 0 builds in
    place); both must give the reference's tree."""
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CANDIDATES_PER_WORLD", "2048")
    _lock_step(layout, mode)


def test_plan_lock_step_empty_last_half(built, monkeypatch):
    """57 worlds: the last wavefront of the 32-lane nodes has one half only."""
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CANDIDATES_PER_WORLD", "2048")
    _lock_step("lattice", "64", worlds=57)


def test_plan_lock_step_without_pillars(built, monkeypatch):
    """No world has pillars: the Pillar table is empty and the candidate scan
    gets a zero-length segment for that archetype."""
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CANDIDATES_PER_WORLD", "2048")
    _lock_step("outlier", "exact", no_pillars=True)


@pytest.mark.parametrize("layout", list(U.LAYOUTS))
def test_plan_segmented_build_equals_the_stack_machine(built, monkeypatch, layout):
    """MADRONA_MWHIP_BVH_CHECK=1: every staged rebuild's breadth-first tree is
    compared word for word with the stack machine's on the same leaves (a
    difference raises kErrPhysics and fails the step), on the tying layouts, in
    lock step with the reference on top."""
    monkeypatch.setenv("MADRONA_MWHIP_BVH_REFRESH", "1")
    monkeypatch.setenv("MADRONA_MWHIP_BVH_CHECK", "1")
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CANDIDATES_PER_WORLD", "2048")
    _lock_step(layout, "64")


def test_plan_lock_step_row_parallel_refresh(built, monkeypatch):
    """MADRONA_MWHIP_BVH_REFRESH=0: the leaf update as a ParallelFor over the
    body rows and the rebuild in a launch of its own."""
    monkeypatch.setenv("MADRONA_MWHIP_BVH_REFRESH", "0")
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CANDIDATES_PER_WORLD", "2048")
    _lock_step("coincident", "64")
