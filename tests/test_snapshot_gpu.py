"""-m gpu: executor snapshots (mwhip_snapshot_*, Simulator.snapshot()).

The oracle is the reference CPU backend stepped through the same inputs (for
navmesh_agents, which has no reference build, the numpy restatement its own
lock-step test uses): a restore followed by K steps must leave EVERY dumped
column and every exported tensor bit for bit where the reference is K steps
after the save point -- floats included.

Inputs are a function of (stream, time), so that a rewound simulator can be
fed the inputs of the time it was rewound to: stream MAIN is what the
reference sees, stream OTHER is what the HIP side is fed between a save and a
restore (with forced resets where the simulator exports a reset tensor), so
that the state just before the restore provably differs from the saved one.

Shapes are the smallest at which a segment copy can still go wrong: one world
(singleton tables hold one row, cleared temporaries none), odd world counts,
every archetype kind (fixed, dynamic with churn, temporaries, singletons,
physics with joints, static data in the persistent region).
"""
import ctypes as C
import os

import numpy as np
import pytest

from madrona_amd.simlib import Simulator, hip_lib_path, ref_lib_path, runtime_lib
from parity_utils import compare_columns

pytestmark = pytest.mark.gpu

MAIN, OTHER = 1000, 2000


def _need_ref(sim):
    if not os.path.exists(ref_lib_path(sim)):
        pytest.skip("oracle/_ref missing on this box")


# ---- inputs as a function of (stream, time) -------------------------------------
def _inputs(sim_name, worlds, stream, t):
    """{tensor name: value} to write before the step that takes time t -> t + 1."""
    rng = np.random.default_rng([stream, t, worlds])
    agents = {"escape_room": 2, "escape_room_phys": 2, "escape_room_render": 2,
              "hideseek": 5}.get(sim_name)
    if agents is not None:
        shape = (worlds, agents)
        grab = sim_name != "escape_room"
        a = np.stack([rng.integers(0, 4, shape), rng.integers(0, 8, shape),
                      rng.integers(-2, 3, shape),
                      rng.integers(0, 2, shape) if grab else np.zeros(shape, int)],
                     -1).astype(np.int32)
        return {"action": a}
    if sim_name == "cartpole":
        return {"action": rng.integers(0, 2, (worlds, 1)).astype(np.int32)}
    return {}


def _feed(sims, sim_name, stream, t, reset=False):
    values = _inputs(sim_name, sims[0].num_worlds, stream, t)
    for s in sims:
        for name, value in values.items():
            s.write_tensor(name, value)
        if reset and "reset" in s.tensor_names:
            s.write_tensor("reset", np.ones((s.num_worlds, 1), np.int32))


def _step(sims, sim_name, stream, t0, n, reset_at=()):
    for t in range(t0, t0 + n):
        _feed(sims, sim_name, stream, t, reset=(t - t0) in reset_at)
        for s in sims:
            s.step(1)


def _tensors_differing(ref, hip):
    return [name for name in ref.tensor_names
            if not np.array_equal(ref.read_tensor(name).view(np.uint8),
                                  hip.read_tensor(name).view(np.uint8))]


def _assert_same(ref, hip, what):
    probs = compare_columns(ref.dump_all(), hip.dump_all())
    assert not probs, (what, probs[:3])
    assert not _tensors_differing(ref, hip), (what, _tensors_differing(ref, hip))


def _assert_dump(ref_dump, hip, what):
    probs = compare_columns(ref_dump, hip.dump_all())
    assert not probs, (what, probs[:3])


def _growths(sim):
    rt = runtime_lib()
    rt.mwhip_num_table_growths.restype = C.c_uint32
    rt.mwhip_num_table_growths.argtypes = [C.c_void_p]
    return rt.mwhip_num_table_growths(sim.hip_exec())


# ---- 1. rewind against the reference ---------------------------------------------
N, M, K = 20, 15, 20
# ball_pit's hinged chains are not stable on the reference itself: positions grow
# ~5x per step and the reference CPU backend stops making progress after a dozen
# steps, well inside the issue's 20 + 20 (test_parity_gpu.py::
# test_ball_pit_hinge_joints pins the first 5 steps for that reason, and says
# so).  That case rewinds inside those 5 steps: save at 2, two other steps,
# restore, three steps -- the reference at 5.  ball_pit exports no reset tensor:
# what the restore has to undo is steps 3 and 4 (asserted to differ from 2).
HINGE_STEPS = (2, 2, 3)

REWIND_CASES = [
    ("cartpole", 3, 0, 5, (N, M, K)),
    ("escape_room", 1, 5, 5, (N, M, K)),
    ("escape_room", 64, 50, 5, (N, M, K)),
    ("escape_room_phys", 16, 40, 5, (N, M, K)),     # grab actions: joints come and go
    ("hideseek", 16, 40, 5, (N, M, K)),
    ("ball_pit", 96, 1 << 24, 5, HINGE_STEPS),      # hinge joints
    ("tgs_drop", 33, 0, 9, (N, M, K)),
    ("sort_stress", 33, 0, 7, (N, M, K)),
    ("sort_stress", 300, 0, 7, (N, M, K)),
    ("mesh_cast", 5, 0, 5, (N, M, K)),      # static trees in the persistent region
]


@pytest.mark.parametrize("sim,worlds,flags,seed,steps", REWIND_CASES)
def test_rewind_against_the_reference(built, sim, worlds, flags, seed, steps):
    _need_ref(sim)
    N, M, K = steps
    with Simulator(ref_lib_path(sim), worlds, seed=seed, num_workers=1, flags=flags) as ref, \
            Simulator(hip_lib_path(sim), worlds, seed=seed, flags=flags) as hip:
        _step([ref, hip], sim, MAIN, 0, N)
        snap = hip.snapshot()
        snap.save()
        assert snap.nbytes > 0
        at_save = hip.dump_all()
        _assert_dump(ref.dump_all(), hip, "save point")

        # another future, on the HIP side only (with two forced resets)
        _step([hip], sim, OTHER, N, M, reset_at=(0, M // 2))
        assert compare_columns(at_save, hip.dump_all()), \
            "the steps between save and restore changed nothing: the test shows nothing"

        snap.restore()
        _assert_dump(at_save, hip, "right after the restore")
        _step([ref, hip], sim, MAIN, N, K)
        _assert_same(ref, hip, f"{N} + {K} steps")
        snap.close()


@pytest.mark.parametrize("worlds", [1, 6])
def test_rewind_navmesh_agents(built, worlds):
    """Navmeshes built by the world constructors in the persistent region; the
    oracle is the numpy restatement (tests/navmesh_restate.py)."""
    import navmesh_restate as R
    seed, flags = 5, 0
    ids = list(range(worlds))

    def check(sim, rest, what):
        dump = sim.dump_all()
        for name, want in rest.columns().items():
            rows, counts = dump[name]
            assert (counts == R.AGENTS_PER_WORLD).all(), (what, name)
            got = rows.view(np.uint32).reshape(len(rows), -1)
            assert np.array_equal(got, want), (what, name)

    with Simulator(hip_lib_path("navmesh_agents"), worlds, seed=seed, flags=flags) as hip:
        rest = R.AgentsRestatement(R.Rand(), hip.lib, ids, seed, flags)
        for _ in range(N):
            hip.step(1)
            rest.step()
        check(hip, rest, "save point")
        with hip.snapshot() as snap:
            snap.save()
            at_save = hip.dump_all()
            hip.step(M)
            assert compare_columns(at_save, hip.dump_all())
            snap.restore()
            for _ in range(K):
                hip.step(1)
                rest.step()
            check(hip, rest, f"{N} + {K} steps")


# ---- 2. save then restore with nothing in between ----------------------------------
@pytest.mark.parametrize("sim,worlds,flags,seed", [("escape_room_phys", 16, 40, 5),
                                                   ("sort_stress", 33, 0, 7),
                                                   ("escape_room", 1, 5, 5)])
def test_save_then_restore_changes_nothing(built, sim, worlds, flags, seed):
    with Simulator(hip_lib_path(sim), worlds, seed=seed, flags=flags) as hip:
        _step([hip], sim, MAIN, 0, 12)
        cap = worlds * 512
        before = [hip.dump_column_raw(i, cap) for i in range(len(hip.columns))]
        tensors = {n: hip.read_tensor(n) for n in hip.tensor_names}
        with hip.snapshot() as snap:
            snap.save()
            first = snap.nbytes
            assert first > 0
            snap.save()
            assert snap.nbytes == first
            snap.restore()
            after = [hip.dump_column_raw(i, cap) for i in range(len(hip.columns))]
            for (name, _, _), b, a in zip(hip.columns, before, after):
                assert b.shape == a.shape and np.array_equal(b, a), name
            for n, value in tensors.items():
                assert np.array_equal(value.view(np.uint8),
                                      hip.read_tensor(n).view(np.uint8)), n
            assert snap.nbytes == first


# ---- 3. two snapshots ------------------------------------------------------------
def test_two_snapshots_are_independent_and_reusable(built):
    sim, worlds, flags = "escape_room_phys", 16, 40
    _need_ref(sim)
    with Simulator(ref_lib_path(sim), worlds, seed=5, num_workers=1, flags=flags) as ref, \
            Simulator(hip_lib_path(sim), worlds, seed=5, flags=flags) as hip:
        want = {}
        for t in range(25):
            _step([ref], sim, MAIN, t, 1)
            if t + 1 in (13, 20, 25):
                want[t + 1] = (ref.dump_all(),
                               {n: ref.read_tensor(n) for n in ref.tensor_names})

        def check(t):
            dump, tensors = want[t]
            _assert_dump(dump, hip, f"time {t}")
            for n, value in tensors.items():
                assert np.array_equal(value.view(np.uint8),
                                      hip.read_tensor(n).view(np.uint8)), (t, n)

        _step([hip], sim, MAIN, 0, 10)
        s1 = hip.snapshot()
        s1.save()
        _step([hip], sim, MAIN, 10, 10)
        s2 = hip.snapshot()
        s2.save()
        check(20)

        s1.restore()
        _step([hip], sim, MAIN, 10, 10)
        check(20)
        s2.restore()
        _step([hip], sim, MAIN, 20, 5)
        check(25)
        s1.restore()
        _step([hip], sim, MAIN, 10, 3)
        check(13)
        s1.close()
        s2.close()


# ---- 4. growth -------------------------------------------------------------------
def test_restore_after_the_tables_grew(built, monkeypatch):
    """sort_stress ramping up from 1 to 40 items per world with tables mapped
    for a quarter of what it declared: the snapshot taken at step 3 is restored
    into tables that have grown since, then saved into again at step 40 (it has
    to make room first)."""
    _need_ref("sort_stress")
    monkeypatch.setenv("MADRONA_MWHIP_INITIAL_CAPACITY_DIV", "4")
    W = 300
    with Simulator(ref_lib_path("sort_stress"), W, seed=7, num_workers=1, flags=2) as ref, \
            Simulator(hip_lib_path("sort_stress"), W, seed=7, flags=2) as hip:
        ref.step(40)
        at_40 = ref.dump_all()
        ref.step(5)
        at_45 = ref.dump_all()

        hip.step(3)
        snap = hip.snapshot()
        snap.save()
        grown = _growths(hip)
        small = snap.nbytes
        hip.step(37)
        assert _growths(hip) > grown, "nothing grew between the save and the restore"
        _assert_dump(at_40, hip, "40 steps, before any restore")
        snap.restore()
        hip.step(37)
        _assert_dump(at_40, hip, "restored to 3, 37 steps")

        snap.save()
        assert snap.nbytes > small
        hip.step(5)
        _assert_dump(at_45, hip, "45 steps")
        snap.restore()
        _assert_dump(at_40, hip, "restored to 40")
        hip.step(5)
        _assert_dump(at_45, hip, "restored to 40, 5 steps")
        snap.close()


def test_restore_after_the_entity_store_and_scratch_grew(built, monkeypatch):
    _need_ref("sort_stress")
    monkeypatch.setenv("MADRONA_MWHIP_INITIAL_ID_CAPACITY_DIV", "64")
    monkeypatch.setenv("MADRONA_MWHIP_TMP_MB", "1")
    W = 6000
    with Simulator(ref_lib_path("sort_stress"), W, seed=3, num_workers=1) as ref, \
            Simulator(hip_lib_path("sort_stress"), W, seed=3) as hip:
        ref.step(16)
        hip.step_async(8)
        hip.sync()
        snap = hip.snapshot()
        snap.save()
        hip.step_async(16)
        hip.sync()
        assert _growths(hip) >= 2
        snap.restore()
        hip.step_async(8)
        hip.sync()
        _assert_dump(ref.dump_all(), hip, "restored to 8, 8 steps")
        snap.close()


def test_save_when_one_low_world_is_a_block_deeper_than_the_rest(built, monkeypatch):
    """The entity store is mapped up to the block a world asked for, not layer
    by layer: with no run-time id blocks provisioned the store ends one block
    behind the singletons' ids, world 0's first item takes exactly that block,
    and the layer it belongs to (one block per world) would end far past the
    mapped slots.  A synchronous save at that replay boundary succeeds and
    holds the slots up to the end of world 0's block."""
    monkeypatch.setenv("MADRONA_MWHIP_ID_BLOCKS_PER_WORLD", "0")
    W, LOAD_PLAN, FLAG_PLAN = 5, 4, 32

    def plan(items):
        p = np.zeros((W, 5), np.int32)
        p[:, 0] = items
        return p

    with Simulator(hip_lib_path("sort_stress"), W, seed=3, flags=FLAG_PLAN) as hip:
        hip.write_tensor("plan", plan([3, 0, 0, 0, 0]))
        hip.run_taskgraph(LOAD_PLAN)
        assert _growths(hip) == 0, "the store grew: world 0 is not at its end"
        snap = hip.snapshot()
        snap.save()
        assert snap.nbytes > 0
        cap = W * 64
        at_save = hip.dump_all()
        raw = [hip.dump_column_raw(i, cap) for i in range(len(hip.columns))]

        hip.write_tensor("plan", plan([1, 0, 0, 0, 0]))
        hip.run_taskgraph(LOAD_PLAN)
        assert compare_columns(at_save, hip.dump_all())
        snap.restore()
        _assert_dump(at_save, hip, "right after the restore")
        for (name, _, _), b, a in zip(
                hip.columns, raw,
                [hip.dump_column_raw(i, cap) for i in range(len(hip.columns))]):
            assert b.shape == a.shape and np.array_equal(b, a), name
        # the restored id cache hands out the same ids, the restored RNG the
        # same items: growing world 0 from the save point gives the same twice
        hip.write_tensor("plan", plan([7, 0, 0, 0, 0]))
        hip.run_taskgraph(LOAD_PLAN)
        first = hip.dump_all()
        hip.write_tensor("plan", plan([2, 0, 0, 0, 0]))
        hip.run_taskgraph(LOAD_PLAN)
        snap.restore()
        hip.write_tensor("plan", plan([7, 0, 0, 0, 0]))
        hip.run_taskgraph(LOAD_PLAN)
        assert not compare_columns(first, hip.dump_all())
        assert _growths(hip) == 0
        snap.close()


# ---- 5. stream order -------------------------------------------------------------
@pytest.mark.parametrize("sim,worlds,seed", [("sort_stress", 300, 7), ("cartpole", 64, 5)])
def test_async_save_and_restore_are_stream_ordered(built, sim, worlds, seed):
    _need_ref(sim)
    with Simulator(ref_lib_path(sim), worlds, seed=seed, num_workers=1) as ref, \
            Simulator(hip_lib_path(sim), worlds, seed=seed) as hip:
        ref.step(16)
        snap = hip.snapshot()
        hip.step_async(8)
        snap.save_async()
        hip.step_async(8)
        snap.restore_async()
        hip.step_async(8)
        hip.sync()
        _assert_same(ref, hip, "8 + save + 8 + restore + 8, one sync")
        snap.close()


def test_restore_does_not_rewind_the_input_ring(built):
    """A restore rewinds the worlds, not the executor's count of replays: the
    replay after it takes the ring slot that follows the last replay's."""
    import torch
    sim, worlds, slots = "escape_room", 300, 5
    ring = np.stack([_inputs(sim, worlds, MAIN, t)["action"] for t in range(slots)])
    with Simulator(hip_lib_path(sim), worlds, seed=3, flags=9) as a, \
            Simulator(hip_lib_path(sim), worlds, seed=3, flags=9) as b:
        dev = torch.from_numpy(ring).cuda()
        a.set_input_ring("action", dev.data_ptr(), slots)
        snap = a.snapshot()
        a.step_async(4)         # slots 0 1 2 3
        snap.save_async()
        a.step_async(3)         # slots 4 0 1
        snap.restore_async()
        a.step_async(6)         # slots 2 3 4 0 1 2 (not 4 0 1 2 3 4)
        a.sync()
        for slot in (0, 1, 2, 3, 2, 3, 4, 0, 1, 2):
            b.write_tensor("action", ring[slot])
            b.step(1)
        assert not compare_columns(a.dump_all(), b.dump_all())
        assert np.array_equal(a.read_tensor("action"), b.read_tensor("action"))
        snap.close()
        del dev


# ---- 6. render -------------------------------------------------------------------
def test_render_after_a_restore_is_the_render_of_the_save_point(built):
    sim, worlds, res = "escape_room_render", 4, 16
    with Simulator(hip_lib_path(sim), worlds, seed=6, flags=9 | (res << 16)) as hip:
        _step([hip], sim, MAIN, 0, 5)
        hip.render()
        rgb, depth = hip.read_tensor("rgb"), hip.read_tensor("depth")
        with hip.snapshot() as snap:
            snap.save()
            _step([hip], sim, OTHER, 5, 10, reset_at=(0,))
            hip.render()
            later_rgb, later_depth = hip.read_tensor("rgb"), hip.read_tensor("depth")
            assert not np.array_equal(depth, later_depth)
            snap.restore()
            # the render outputs are not part of a snapshot: until the next
            # render pass they show what was rendered last
            assert np.array_equal(hip.read_tensor("rgb"), later_rgb)
            assert np.array_equal(hip.read_tensor("depth").view(np.uint32),
                                  later_depth.view(np.uint32))
            hip.render()
            assert np.array_equal(hip.read_tensor("rgb"), rgb)
            assert np.array_equal(hip.read_tensor("depth").view(np.uint32),
                                  depth.view(np.uint32))


# ---- 7. refusals -----------------------------------------------------------------
def _refused(rt, call, exec_, handle, state_of):
    before = state_of.dump_all()
    rc = call(exec_, handle)
    assert rc != 0
    assert len(rt.mwhip_last_error()) > 0
    state_of.sync()
    assert not compare_columns(before, state_of.dump_all())
    return rt.mwhip_last_error().decode()


def test_refusals(built, monkeypatch):
    rt = runtime_lib()
    with Simulator(hip_lib_path("escape_room"), 5, seed=5, flags=5) as a, \
            Simulator(hip_lib_path("escape_room"), 5, seed=5, flags=5) as b:
        _step([a, b], "escape_room", MAIN, 0, 6)
        empty = a.snapshot()
        for call in (rt.mwhip_snapshot_restore, rt.mwhip_snapshot_restore_async):
            text = _refused(rt, call, a.hip_exec(), empty.handle, a)
            assert "never saved" in text
        # a handle of another executor: refused by b, whatever the call
        mine = a.snapshot()
        mine.save()
        _step([b], "escape_room", OTHER, 6, 2)
        for call in (rt.mwhip_snapshot_restore, rt.mwhip_snapshot_restore_async,
                     rt.mwhip_snapshot_save, rt.mwhip_snapshot_save_async):
            text = _refused(rt, call, b.hip_exec(), mine.handle, b)
            assert "not one of this executor's" in text
        mine.restore()          # (its own executor takes it)
        empty.close()
        mine.close()

    # an asynchronous save that finds a table larger than the room the snapshot
    # was given: sort_stress ramping up, tables mapped for a sixteenth of what it
    # declared (the first step already outruns that), snapshot sized before it
    monkeypatch.setenv("MADRONA_MWHIP_INITIAL_CAPACITY_DIV", "16")
    with Simulator(hip_lib_path("sort_stress"), 300, seed=7, flags=2) as s:
        snap = s.snapshot()
        snap.save()
        s.step(12)
        snap.save_async()
        s.sync()
        for call in (rt.mwhip_snapshot_restore, rt.mwhip_snapshot_restore_async):
            text = _refused(rt, call, s.hip_exec(), snap.handle, s)
            assert "save into it again" in text
        # ... and is whole again after a save that makes room
        snap.save()
        at_save = s.dump_all()
        s.step(3)
        snap.restore()
        assert not compare_columns(at_save, s.dump_all())
        snap.close()


def test_a_snapshot_that_outlives_its_simulator_is_empty(built):
    """Simulator.close() frees the executor's snapshots: the Python objects left
    over never pass the dead executor on."""
    with Simulator(hip_lib_path("cartpole"), 3, seed=5) as hip:
        hip.step(2)
        snap = hip.snapshot()
        snap.save()
    assert snap.handle == 0
    with pytest.raises(RuntimeError):
        snap.restore()
    with pytest.raises(RuntimeError):
        snap.nbytes
    snap.close()


def test_a_restore_queued_behind_an_overflowed_save_is_reported(built, monkeypatch):
    """restore_async right behind a save_async that finds a table larger than
    the snapshot's room: the host may not know yet, so the call may be accepted
    -- its kernel then moves nothing and raises kErrSnapshot, which the next
    sync() reports.  Either way the caller is told; never a silent no-op."""
    monkeypatch.setenv("MADRONA_MWHIP_INITIAL_CAPACITY_DIV", "16")
    with Simulator(hip_lib_path("sort_stress"), 300, seed=7, flags=2) as s:
        snap = s.snapshot()
        snap.save()
        s.step(12)
        before = s.dump_all()
        snap.save_async()
        try:
            snap.restore_async()
        except RuntimeError as e:
            assert "save into it again" in str(e)
            s.sync()
        else:
            with pytest.raises(RuntimeError, match="snapshot restore was skipped"):
                s.sync()
        assert not compare_columns(before, s.dump_all())
        snap.close()
