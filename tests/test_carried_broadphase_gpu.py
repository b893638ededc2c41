"""-m gpu: the carried-over broadphase (PhysicsSystem::BroadphaseInputs::CarriedOver,
MWHIP_NODE_CARRIED, MADRONA_MWHIP_CARRY_BROADPHASE).

A replay that directly follows a replay of the same launch graph leaves out the
step's first leaf refresh.  The yardstick is the same binary with every replay
full (MADRONA_MWHIP_CARRY_BROADPHASE=0): every dumped column and every exported
tensor must be the same bits.  Actions come from a device-resident input ring,
as in bench.py: a host write of the action tensor between two steps is an entry
point that makes the next replay a full one, and nothing would be carried.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib

pytestmark = pytest.mark.gpu

ENV = "MADRONA_MWHIP_CARRY_BROADPHASE"
STEPS = 40
AGENTS = {"escape_room_phys": 2, "hideseek": 5}
# sims/broadphase_only/sim.hpp, plan::flagCarried...
BP_CARRIED, BP_NUDGE, BP_EXPORT = 1 << 12, 1 << 13, 1 << 15

# escape_room_phys at 3 and 65 worlds, hideseek at 3 and 16; a world resets with
# probability 1 in 3 and 1 in 40 per step
CASES = [("escape_room_phys", 3, 3), ("escape_room_phys", 3, 40),
         ("escape_room_phys", 65, 3), ("escape_room_phys", 65, 40),
         ("hideseek", 3, 3), ("hideseek", 3, 40),
         ("hideseek", 16, 3), ("hideseek", 16, 40)]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _action_ring(sim, worlds, slots=STEPS, seed=17):
    """[slots, worlds, agents, 4]: move amount, angle, rotate, grab (pressed half
    of the time)"""
    rng = np.random.default_rng(seed)
    A = AGENTS[sim]
    return np.stack([np.stack([rng.integers(0, 4, (worlds, A)), rng.integers(0, 8, (worlds, A)),
                               rng.integers(-2, 3, (worlds, A)), rng.integers(0, 2, (worlds, A))],
                              -1) for _ in range(slots)]).astype(np.int32)


def _state(s):
    """every dumped column (rows and per-world counts) and every exported tensor"""
    state = {}
    for name, (rows, counts) in s.dump_all(512).items():
        state["col:" + name] = rows
        state["cnt:" + name] = counts
    for name in s.tensor_names:
        state["tensor:" + name] = s.read_tensor(name)
    return state


def _same(got, want, what):
    assert list(got) == list(want), what
    for name in want:
        assert got[name].shape == want[name].shape, (what, name)
        assert got[name].tobytes() == want[name].tobytes(), (what, name, "bits differ")


def _set_mode(mode):
    if mode is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = str(mode)


@pytest.fixture(autouse=True)
def _restore_env():
    before = os.environ.get(ENV)
    yield
    _set_mode(before)


@functools.lru_cache(maxsize=None)
def _rollout(sim, worlds, denom, mode, one_by_one=False):
    """STEPS steps of `sim` under MADRONA_MWHIP_CARRY_BROADPHASE=mode (None: unset)
    -> (state, counters); computed once and shared, never modified"""
    torch = _torch()
    _set_mode(mode)
    with Simulator(hip_lib_path(sim), worlds, seed=5, flags=denom) as s:
        ring = torch.from_numpy(_action_ring(sim, worlds)).cuda()
        torch.cuda.synchronize()
        s.set_input_ring("action", ring.data_ptr(), STEPS)
        if one_by_one:
            for _ in range(STEPS):
                s.step_async(1)
                s.sync()
        else:
            s.step_async(STEPS)
            s.sync()
        return _state(s), s.broadphase_stats()


def _mostly_carried(counts, steps):
    """The first replay is full; so is the one behind each rebuild of the launch
    graphs (a table that grew), of which a run this short has a few at most."""
    assert counts["carried_replays"] + counts["full_replays"] == steps, counts
    assert 1 <= counts["full_replays"] <= 4, counts


# ---- 1. same bits with and without ------------------------------------------------------
@pytest.mark.parametrize("sim,worlds,denom", CASES)
def test_same_bits_with_and_without(built, sim, worlds, denom):
    full, full_counts = _rollout(sim, worlds, denom, 0)
    assert full_counts == {"carried_replays": 0, "full_replays": STEPS}
    carried, counts = _rollout(sim, worlds, denom, None)
    # (the first replay after creation -- and after the ring was set -- is full)
    _mostly_carried(counts, STEPS)
    _same(carried, full, (sim, worlds, denom, "default against =0"))
    stepped, counts = _rollout(sim, worlds, denom, None, one_by_one=True)
    # (mwhip_synchronize between two replays changes nothing)
    _mostly_carried(counts, STEPS)
    _same(stepped, carried, (sim, worlds, denom, "forty step_async(1) against step_async(40)"))


# ---- 2. check mode is silent --------------------------------------------------------------
@pytest.mark.parametrize("sim,worlds,denom", CASES)
def test_check_mode_is_silent(built, sim, worlds, denom):
    """=2: the refresh that would be left out compares instead of storing, every
    replay counts as full; sync() inside _rollout raises on kErrPhysics"""
    checked, counts = _rollout(sim, worlds, denom, 2)
    assert counts == {"carried_replays": 0, "full_replays": STEPS}
    full, _ = _rollout(sim, worlds, denom, 0)
    _same(checked, full, (sim, worlds, denom, "=2 against =0"))


# ---- 3. check mode speaks -----------------------------------------------------------------
def _broadphase_only(flags, steps, worlds=5):
    with Simulator(hip_lib_path("broadphase_only"), worlds, seed=9, flags=flags) as s:
        s.step_async(steps)
        s.sync()
        return _state(s), s.broadphase_stats()


def test_check_mode_finds_a_broken_promise(built):
    """broadphase_only with a CarriedOver broadphase in front of its drift.  A
    node in front of that one moves each world's first box: the check raises the
    executor's device error at the second replay (the first one is full)."""
    _set_mode(2)
    with pytest.raises(RuntimeError, match=r"-5.*device error"):
        _broadphase_only(BP_CARRIED | BP_NUDGE, 4)
    # the same graph without the node: silent, over a rebuild (every 16 steps)
    checked, counts = _broadphase_only(BP_CARRIED, 20)
    assert counts == {"carried_replays": 0, "full_replays": 20}
    _set_mode(0)
    full, _ = _broadphase_only(BP_CARRIED, 20)
    _same(checked, full, "broadphase_only, =2 against =0")
    _set_mode(None)
    carried, counts = _broadphase_only(BP_CARRIED, 20)
    _mostly_carried(counts, 20)
    _same(carried, full, "broadphase_only, default against =0")


# ---- 4. the full variant runs when it must ------------------------------------------------
def _pair(worlds=65, denom=40):
    """escape_room_phys twice, driven by the same ring: default, and =0"""
    torch = _torch()
    ring = torch.from_numpy(_action_ring("escape_room_phys", worlds)).cuda()
    torch.cuda.synchronize()
    sims = []
    for mode in (None, 0):
        _set_mode(mode)
        s = Simulator(hip_lib_path("escape_room_phys"), worlds, seed=5, flags=denom)
        s._ring = ring
        s.set_input_ring("action", ring.data_ptr(), STEPS)
        sims.append(s)
    return sims


def _next_replay_is_full(a, b, what):
    """one step: a's replay ran everything; four more: nine... all carried; then
    both simulators hold the same bits"""
    before = a.broadphase_stats()
    for s in (a, b):
        s.step_async(1)
        s.sync()
    after = a.broadphase_stats()
    assert after == {"carried_replays": before["carried_replays"],
                     "full_replays": before["full_replays"] + 1}, what
    for s in (a, b):
        s.step_async(4)
        s.sync()
    assert a.broadphase_stats() == {"carried_replays": after["carried_replays"] + 4,
                                    "full_replays": after["full_replays"]}, what
    _same(_state(a), _state(b), (what, "5 steps later"))


def test_full_replay_after_restore_teleport_and_another_graph(built):
    torch = _torch()
    a, b = _pair()
    try:
        for s in (a, b):
            s.step_async(10)
            s.sync()
        assert a.broadphase_stats() == {"carried_replays": 9, "full_replays": 1}
        assert b.broadphase_stats() == {"carried_replays": 0, "full_replays": 10}
        _same(_state(a), _state(b), "10 steps")

        # a snapshot restore (the save is an entry point of its own: it makes a
        # replay full as well, so steps run between the two)
        snaps = [s.snapshot() for s in (a, b)]
        for s, snap in zip((a, b), snaps):
            snap.save()
            s.step_async(3)
            s.sync()
            snap.restore()
        _next_replay_is_full(a, b, "a snapshot restore")

        # a world write that teleports the bodies of two worlds: lidar, grab
        # results and everything else are in _state.  (Views, writes and the
        # probe graph below are made first and steps run behind that: making
        # them is an entry point of its own.)
        moved = [1, 40]
        name = "PhysicsEntity.Position"
        rows = int(a.dump_all(512)[name][1].max())
        views = [s.world_view("PhysicsEntity", [name], max_rows=rows + 2) for s in (a, b)]
        writes = [s.world_write("PhysicsEntity", [name], max_rows=rows + 2) for s in (a, b)]
        probes = [s.taskgraph_graph(0) for s in (a, b)]
        for s, view, write in zip((a, b), views, writes):
            view.compute()
            write.tensor(name).copy_(view.tensor(name))
            write.tensor(name, np.float32)[moved, :, 0] += 0.25
            take = torch.zeros(s.num_worlds, dtype=torch.int32, device="cuda")
            take[moved] = write.max_rows
            write.take.copy_(take)
        torch.cuda.synchronize()
        for s, write in zip((a, b), writes):
            s.step_async(2)
            s.sync()
            write.apply()
        _next_replay_is_full(a, b, "a teleporting world write")

        # a replay of another launch graph (the launch graph of task graph 0
        # alone: another handle)
        for s, probe in zip((a, b), probes):
            s.step_async(1, graph=probe)
            s.sync()
        _next_replay_is_full(a, b, "a replay of another launch graph")
        for obj in snaps + views + writes:
            obj.close()
    finally:
        a.close()
        b.close()


def test_every_replay_is_full_with_a_step_write_or_an_exported_position(built):
    torch = _torch()
    _set_mode(None)
    with Simulator(hip_lib_path("escape_room_phys"), 65, seed=5, flags=40) as s:
        name = "PhysicsEntity.Position"
        with s.world_write("PhysicsEntity", [name], max_rows=4) as write:
            write.take.zero_()          # (writes nothing; it could)
            torch.cuda.synchronize()
            write.every_step()
            s.step_async(6)
            s.sync()
            assert s.broadphase_stats() == {"carried_replays": 0, "full_replays": 6}
            write.every_step(False)
            s.step_async(6)
            s.sync()
            # (carried again; full: the one behind the unset, and the one behind
            # each rebuild for a table that grew in these early steps)
            counts = s.broadphase_stats()
            assert counts["carried_replays"] + counts["full_replays"] == 12, counts
            assert 7 <= counts["full_replays"] <= 9, counts
    _, counts = _broadphase_only(BP_CARRIED | BP_EXPORT, 6)
    assert counts == {"carried_replays": 0, "full_replays": 6}
    _, counts = _broadphase_only(BP_CARRIED, 6)
    assert counts == {"carried_replays": 5, "full_replays": 1}


# ---- 5. build-time refusal ----------------------------------------------------------------
class _NodeDesc(C.Structure):
    """mwhip_node_desc (include/mwhip.h)"""
    _fields_ = [("kind", C.c_uint32), ("name", C.c_char_p), ("kernel", C.c_void_p),
                ("wants_pfor_args", C.c_uint32), ("node_data_id", C.c_int32),
                ("arg0", C.c_uint32), ("arg1", C.c_uint32), ("count_mode", C.c_uint32),
                ("fixed_count", C.c_uint32), ("threads_per_invocation", C.c_uint32),
                ("query_offset", C.c_uint32), ("num_matching", C.c_uint32),
                ("bytes_per_row", C.c_uint32), ("archetype_id", C.c_uint32),
                ("component_id", C.c_uint32), ("io_declared", C.c_uint32),
                ("pfor_body", C.c_void_p), ("write_mask", C.c_uint32),
                ("pfor_group_kernel", C.c_void_p)]


MWHIP_NODE_KERNEL, MWHIP_NODE_CARRIED, MWHIP_COUNT_PER_WORLD = 0, 0x80000000, 2


def test_a_task_graph_with_nothing_to_carry_over_is_refused(built):
    """A carried leaf refresh BEHIND the task graph's only broadphase: no unflagged
    node of its name follows it, so building a launch graph from the task graph
    fails with the message.  (Through the C ABI: the C++ shim aborts on a failed
    build, as the reference's executor does on its own errors.  The refusal comes
    before anything is instantiated: the node's kernel is never looked at.)"""
    _set_mode(None)
    rt = runtime_lib()
    rt.mwhip_tg_add_node.restype = C.c_int32
    rt.mwhip_tg_add_node.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_NodeDesc),
                                     C.POINTER(C.c_int32), C.c_uint32]
    rt.mwhip_build_launch_graph.restype = C.c_int32
    rt.mwhip_build_launch_graph.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32,
                                            C.c_char_p, C.POINTER(C.c_uint64)]
    with Simulator(hip_lib_path("broadphase_only"), 5, seed=9) as s:
        s.step(2)
        before = _state(s)
        desc = _NodeDesc()
        desc.kind = MWHIP_NODE_KERNEL | MWHIP_NODE_CARRIED
        desc.name = b"physics:bvhRefresh+rebuild"
        desc.kernel = 1             # (non-null; never launched)
        desc.node_data_id = -1
        desc.count_mode = MWHIP_COUNT_PER_WORLD
        desc.threads_per_invocation = 64
        assert rt.mwhip_tg_add_node(s.hip_exec(), 0, C.byref(desc), None, 0) >= 0
        ids, out = (C.c_uint32 * 1)(0), C.c_uint64(0)
        rc = rt.mwhip_build_launch_graph(s.hip_exec(), ids, 1, None, C.byref(out))
        message = rt.mwhip_last_error().decode()
        assert rc == -3 and out.value == 0, (rc, message)
        assert "physics:bvhRefresh+rebuild" in message and \
            "nothing to carry over" in message, message
        # the step graph built before is what it was
        _same(_state(s), before, "after the refused build")
