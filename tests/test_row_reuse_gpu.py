"""-m gpu: row reuse of the ordered create / destroy (OrderedRows::Reuse,
madrona/state.inl) and the world sort that finds its table refilled in place
(csrc/sort_archetype.hip, tableRefilled).

Lock step with the reference CPU backend, every step bit for bit: every dumped
column (entity ids and generations are the Entity columns), rows per world, and
at the end every exported tensor.  Every case runs with reuse and with
MADRONA_MWHIP_ROW_REUSE=0, which must be the same simulator step for step.

sims/sort_stress with flags 128 (Config::reusePlan) walks the rule off the happy
path: whole range / proper suffix with as many, fewer and more creates, a subset
that is no suffix, two and five archetypes in one call, worlds without rows --
next to the usual Item churn (plain destroys) on another table."""
import ctypes as C
import os

import numpy as np
import pytest

from madrona_amd.simlib import Simulator, hip_lib_path, ref_lib_path
from parity_utils import compare_columns, run_pair

pytestmark = pytest.mark.gpu

REUSE_PLAN = 128
SWITCH = "MADRONA_MWHIP_ROW_REUSE"


def _need_ref(sim):
    if not os.path.exists(ref_lib_path(sim)):
        pytest.skip("oracle/_ref missing on this box")


def _need_plan_mode():
    _need_ref("sort_stress")
    with Simulator(ref_lib_path("sort_stress"), 1, seed=7, num_workers=1,
                   flags=REUSE_PLAN) as ref:
        names = [name for name, _, _ in ref.columns]
    if "Reuse0.Key" not in names:
        pytest.skip("reference backend of sort_stress built from sources without "
                    "the reuse plan mode")


def _switch(monkeypatch, reuse):
    if reuse:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, "0")


def _actions(seed, agents):
    rng = np.random.default_rng(seed)

    def feed(ref, hip, step):
        shape = (ref.num_worlds, agents)
        # (grab pressed half the time)
        a = np.stack([rng.integers(0, 4, shape), rng.integers(0, 8, shape),
                      rng.integers(-2, 3, shape), rng.integers(0, 2, shape)],
                     -1).astype(np.int32)
        ref.write_tensor("action", a)
        hip.write_tensor("action", a)
    return feed


def _archetype_of(sim, column):
    names = [name for name, _, _ in sim.columns]
    arch, comp = C.c_uint32(0), C.c_uint32(0)
    assert sim.lib.sim_hip_column_ids(sim.handle, names.index(column), C.byref(arch),
                                      C.byref(comp)) == 0
    return arch.value


REUSE = pytest.mark.parametrize("reuse", [True, False], ids=["reuse", "switch_off"])


# ---- the rule away from the happy path ------------------------------------------
@REUSE
@pytest.mark.parametrize("worlds", [1, 2, 3, 65])
def test_sort_stress_plan_lockstep(built, monkeypatch, worlds, reuse):
    _need_plan_mode()
    _switch(monkeypatch, reuse)
    probs, step = run_pair("sort_stress", worlds, 24, seed=7, flags=REUSE_PLAN)
    assert not probs, (step, probs[:3])


def test_sort_stress_plan_takes_every_path(built, monkeypatch):
    """Over the plan's cycle the first table is refilled in place in some steps
    and sorted in others; with the switch off nothing is reused or skipped."""
    _need_plan_mode()
    for reuse in (True, False):
        _switch(monkeypatch, reuse)
        with Simulator(hip_lib_path("sort_stress"), 16, seed=7, flags=REUSE_PLAN) as s:
            s.step(24)
            stats = s.sort_stats()
            first = stats[_archetype_of(s, "Reuse0.Key")]
        if reuse:
            assert first["rows_reused"] > 0 and first["runs"] > 1, first
            assert first["skipped_runs"] == 0 or first["runs"] > 1, first
        else:
            assert all(st["rows_reused"] == 0 and st["skipped_runs"] == 0
                       for st in stats.values()), stats


def test_a_fifth_archetype_gets_no_record(built, monkeypatch):
    """One world with global index 1: it starts with 3, 5, 1, 3, 5 rows in the five
    tables, its first five steps touch the first two only, and its sixth (plan
    kind 6) destroys the last row of each table and creates one in each.  The
    first four get a record and are refilled in place; the fifth archetype of
    the call has none: a plain hole and an appended row, its table is sorted."""
    _need_plan_mode()
    _switch(monkeypatch, True)
    with Simulator(hip_lib_path("sort_stress"), 1, seed=7, flags=REUSE_PLAN,
                   world_base=1) as s:
        archs = [_archetype_of(s, f"Reuse{a}.Key") for a in range(5)]
        s.step(5)
        before = s.sort_stats()
        counts = [int(s.dump_all()[f"Reuse{a}.Key"][1][0]) for a in range(5)]
        assert min(counts) >= 1, counts
        s.step(1)
        after = s.sort_stats()
        assert [int(s.dump_all()[f"Reuse{a}.Key"][1][0]) for a in range(5)] == counts
    for a, arch in enumerate(archs):
        d = {k: after[arch][k] - before[arch][k] for k in after[arch]}
        if a < 4:
            assert (d["rows_reused"], d["skipped_runs"], d["runs"]) == (1, 1, 0), (a, d)
        else:
            assert (d["rows_reused"], d["skipped_runs"], d["runs"]) == (0, 0, 1), (a, d)


def test_plain_destroy_next_to_resets_runs_the_chain(built, monkeypatch):
    """8 worlds, step 1 of the plan: worlds 0 .. 3 and 7 replace a suffix of
    their Reuse0 rows, world 4 adds two, world 3 (kind 4) destroys its FIRST row
    -- a hole no create refills: the table is sorted, not skipped, and still
    equals the reference's (lock-step test above, same flags)."""
    _need_plan_mode()
    _switch(monkeypatch, True)
    with Simulator(hip_lib_path("sort_stress"), 8, seed=7, flags=REUSE_PLAN) as s:
        arch = _archetype_of(s, "Reuse0.Key")
        s.step(1)               # cold: sorts
        before = s.sort_stats()[arch]
        s.step(1)
        after = s.sort_stats()[arch]
    assert after["runs"] == before["runs"] + 1, (before, after)
    assert after["skipped_runs"] == before["skipped_runs"], (before, after)
    assert after["rows_reused"] > before["rows_reused"], (before, after)


# ---- the three simulators whose reset systems opt in ----------------------------
@REUSE
@pytest.mark.parametrize("denom", [3, 40])
@pytest.mark.parametrize("worlds", [1, 3, 65])
def test_escape_room_phys_lockstep(built, monkeypatch, worlds, denom, reuse):
    _need_ref("escape_room_phys")
    _switch(monkeypatch, reuse)
    probs, step = run_pair("escape_room_phys", worlds, 40, flags=denom,
                           actions=_actions(worlds + denom, 2), check_init=False)
    assert not probs, (step, probs[:3])


@REUSE
@pytest.mark.parametrize("worlds", [3, 65])
def test_escape_room_lockstep(built, monkeypatch, worlds, reuse):
    _need_ref("escape_room")
    _switch(monkeypatch, reuse)
    probs, step = run_pair("escape_room", worlds, 40, flags=3,
                           actions=_actions(worlds, 2), check_init=False)
    assert not probs, (step, probs[:3])


@REUSE
@pytest.mark.parametrize("worlds", [3, 16])
def test_hideseek_lockstep(built, monkeypatch, worlds, reuse):
    _need_ref("hideseek")
    _switch(monkeypatch, reuse)
    probs, step = run_pair("hideseek", worlds, 40, flags=3,
                           actions=_actions(worlds, 5), check_init=False)
    assert not probs, (step, probs[:3])


@REUSE
def test_every_world_resets_in_the_same_step(built, monkeypatch, reuse):
    """Steps 1, 5 and 6."""
    _need_ref("escape_room_phys")
    _switch(monkeypatch, reuse)
    W = 65
    feed = _actions(9, 2)

    def actions(ref, hip, step):
        feed(ref, hip, step)
        if step in (1, 5, 6):
            for s in (ref, hip):
                s.write_tensor("reset", np.ones((W, 1), np.int32))

    probs, step = run_pair("escape_room_phys", W, 10, flags=0, actions=actions,
                           check_init=False)
    assert not probs, (step, probs[:3])


# ---- the sort node's counters ---------------------------------------------------
RESETS = {1: range(0, 65, 2), 3: [7], 4: range(65), 6: [0, 64], 7: [0, 64], 9: range(10, 30)}


@REUSE
def test_refilled_tables_are_skipped(built, monkeypatch, reuse):
    """escape_room_phys, 65 worlds, no random resets: the body, door and button
    tables change only where the reset tensor says so.  A step with resets is
    skipped by all three tables and reuses exactly the rows the resetting worlds
    replaced; a step without resets is neither run nor skipped.  With the switch
    off every reset step runs the chain.  (The executor world-sorts every table
    once when it is created, the counters say so below: this simulator has no
    cold first step.  test_table_never_world_sorted_reuses_nothing is the cold
    case.)"""
    _switch(monkeypatch, reuse)
    W = 65
    feed = _actions(4, 2)
    with Simulator(hip_lib_path("escape_room_phys"), W, seed=5, flags=0) as s:
        tables = {t: _archetype_of(s, f"{t}.Entity")
                  for t in ("PhysicsEntity", "DoorEntity", "ButtonEntity")}
        last = {t: s.sort_stats()[a] for t, a in tables.items()}
        for t, st in last.items():
            assert st["runs"] == 1 and st["skipped_runs"] == 0 and st["rows_reused"] == 0, (t, st)
        # rows of a world's level per table: what a reset replaces
        level_rows = {}
        dump = s.dump_all()
        for t in tables:
            counts = dump[f"{t}.Entity"][1]
            assert (counts == counts[0]).all()
            level_rows[t] = int(counts[0])
        level_rows["PhysicsEntity"] -= 1 + 4    # floor and borders stay
        assert level_rows == {"PhysicsEntity": 18, "DoorEntity": 3, "ButtonEntity": 6}
        for step in range(1, 11):
            feed(s, s, step)
            resetting = list(RESETS.get(step, []))
            if resetting:
                r = np.zeros((W, 1), np.int32)
                r[resetting] = 1
                s.write_tensor("reset", r)
            s.step(1)
            stats = s.sort_stats()
            for t, arch in tables.items():
                now, was = stats[arch], last[t]
                d = {k: now[k] - was[k] for k in now}
                what = (step, t, d)
                if not resetting:
                    assert d["runs"] == 0 and d["skipped_runs"] == 0, what
                elif reuse:
                    assert d["runs"] == 0 and d["skipped_runs"] == 1, what
                    assert d["rows_reused"] == len(resetting) * level_rows[t], what
                else:
                    assert d["runs"] == 1 and d["skipped_runs"] == 0, what
                    assert d["rows_reused"] == 0, what
                last[t] = now


REUSE_PLAN_ONLY = 9     # sort_stress: reusePlanSystem without the compactions


def test_table_never_world_sorted_reuses_nothing(built, monkeypatch):
    """One world with global index 6 (plan kind 6 while its step counter stands
    still: the last row of every table goes, one row comes).  It starts with
    0, 2, 4, 0, 2 rows: the first and fourth table are empty when the executor
    sorts every table at creation, so they have no sorted prefix.  Two runs of the
    plan WITHOUT compaction: the rows the first run appended to those two tables
    are destroyed by the second, a suffix of the world's rows in a table that was
    never world-sorted: nothing is remembered, the new rows are appended.  The
    other three reuse.  The step that follows sorts all five; every column
    equals the same sequence with the switch off."""
    _need_plan_mode()
    dumps, stats = {}, {}
    for reuse in (True, False):
        _switch(monkeypatch, reuse)
        with Simulator(hip_lib_path("sort_stress"), 1, seed=7, flags=REUSE_PLAN,
                       world_base=6) as s:
            archs = [_archetype_of(s, f"Reuse{a}.Key") for a in range(5)]
            counts = [int(s.dump_all()[f"Reuse{a}.Key"][1][0]) for a in range(5)]
            assert counts == [0, 2, 4, 0, 2]
            s.run_taskgraph(REUSE_PLAN_ONLY)
            s.run_taskgraph(REUSE_PLAN_ONLY)
            st = s.sort_stats()
            before = [dict(st[a]) for a in archs]
            s.step(1)
            st = s.sort_stats()
            stats[reuse] = [{k: st[a][k] - b[k] for k in b} for a, b in zip(archs, before)]
            dumps[reuse] = s.dump_all()
    for a in range(5):
        d = stats[True][a]
        if a in (0, 3):
            # (the step's own plan run finds the appended rows unsorted again)
            assert d["rows_reused"] == 0 and d["skipped_runs"] == 0 and d["runs"] == 1, (a, d)
        else:
            assert d["rows_reused"] >= 2, (a, d)
        assert stats[False][a]["rows_reused"] == 0 and stats[False][a]["skipped_runs"] == 0
    for name, (rows, counts) in dumps[False].items():
        assert np.array_equal(counts, dumps[True][name][1]), name
        assert np.array_equal(rows, dumps[True][name][0]), name


# ---- snapshots ------------------------------------------------------------------
def test_snapshot_around_a_step_with_resets(built, monkeypatch):
    """Saved between a step whose resets reused rows and the next one, restored
    after three more steps with other inputs and forced resets: the steps after
    the restore equal the uninterrupted run's."""
    _switch(monkeypatch, True)
    W = 33

    def feed(s, stream, t, reset=()):
        rng = np.random.default_rng([stream, t])
        shape = (W, 2)
        a = np.stack([rng.integers(0, 4, shape), rng.integers(0, 8, shape),
                      rng.integers(-2, 3, shape), rng.integers(0, 2, shape)],
                     -1).astype(np.int32)
        s.write_tensor("action", a)
        if len(reset):
            r = np.zeros((W, 1), np.int32)
            r[list(reset)] = 1
            s.write_tensor("reset", r)

    main_resets = {3: range(0, W, 3), 4: [1, 2], 6: range(W), 8: [5]}
    with Simulator(hip_lib_path("escape_room_phys"), W, seed=5, flags=0) as whole, \
            Simulator(hip_lib_path("escape_room_phys"), W, seed=5, flags=0) as s, \
            s.snapshot() as snap:
        for t in range(1, 5):
            for sim in (whole, s):
                feed(sim, 1, t, main_resets.get(t, ()))
                sim.step(1)
        snap.save()
        for t in range(5, 8):
            feed(s, 2, t, range(0, W, 2))
            s.step(1)
        snap.restore()
        for t in range(5, 10):
            for sim in (whole, s):
                feed(sim, 1, t, main_resets.get(t, ()))
                sim.step(1)
            probs = compare_columns(whole.dump_all(), s.dump_all())
            assert not probs, (t, probs[:3])
        for name in whole.tensor_names:
            assert np.array_equal(whole.read_tensor(name).view(np.uint8),
                                  s.read_tensor(name).view(np.uint8)), name
