"""Contact queries (mwhip_contacts_*, Simulator.contact_query) on
the device.  The yardsticks are not the code under test: madrona_amd/contact_ref.py
with the reference's own scalar narrowphase (ref_collide_pair of
oracle/_ref/libphys_ref.so) over the dumps of the contact_probe simulator, which
is first shown to be in lock step with the reference backend; the brute force of
tests/contact_utils.py; and the plain mapping -- the generic single-lane routine,
pair after pair -- for the cooperative one on shapes the oracle cannot judge."""
import ctypes as C
import os

import numpy as np
import pytest

import contact_utils as cu
from conftest import ref_available
from madrona_amd import contact_ref as cr
from madrona_amd.simlib import (RING_ON_STEP, ContactsDesc, Simulator, hip_lib_path,
                                ref_lib_path, runtime_lib)
from parity_utils import compare_columns

pytestmark = pytest.mark.gpu

W, K = cu.PROBE_WORLDS, cu.MAX_CONTACTS
REST_WINDOW = range(111, 121)       # ten consecutive steps late enough for bodies to rest
NAMES = ("status", "count", "pairs", "num_points", "normal", "points")
LAUNCH = "contacts:contacts"
UNCUT = 512     # slots enough for every contact of the crowded pen


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _out(q):
    _torch().cuda.synchronize()
    return {"status": q.status().cpu().numpy(), "count": q.counts().cpu().numpy(),
            "pairs": q.pairs().cpu().numpy(), "num_points": q.num_points().cpu().numpy(),
            "normal": q.normals().cpu().numpy(), "points": q.points().cpu().numpy()}


def _same(a, b, what):
    """bit for bit, order included"""
    for name in NAMES:
        x, y = a[name], b[name]
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        bad = np.argwhere(x != y)
        assert bad.size == 0, (what, name, bad[:4].tolist())


def _probe(worlds=W):
    return Simulator(hip_lib_path("contact_probe"), worlds, seed=cu.PROBE_SEED)


def _needs_oracle():
    if not (ref_available("contact_probe") and os.path.exists(cu.PHYS_REF)):
        pytest.skip("oracle/_ref not built here (no reference tree)")


@pytest.fixture(scope="module")
def oracle(built):
    _needs_oracle()
    lib = cu.phys_ref()
    return lib, cu.probe_objects(lib)


@pytest.fixture(scope="module")
def run(built):
    """The HIP probe stepped through REST_WINDOW once: at every compared step
    its dump and what the solver-pose and current-pose queries computed; over
    the window every body's speed and the solver-pose contacts (uncut)."""
    record, window = {}, []
    with _probe() as sim:
        solver, current = sim.contact_query(K), sim.contact_query(K, poses="current")
        uncut = sim.contact_query(UNCUT)
        for step in range(1, max(REST_WINDOW) + 1):
            sim.step(1)
            if step in cu.STEPS:
                record[step] = (sim.dump_all(), _out(solver.compute()), _out(current.compute()))
            if step in REST_WINDOW:
                dump = sim.dump_all()
                window.append((dump["Body.Entity"][0].view(np.int32).copy(),
                               dump["Body.Velocity"][0].view(np.float32)[:, :3].copy(),
                               dump["Body.ResponseType"][0].view(np.int32)[:, 0].copy(),
                               _out(uncut.compute())))
    return record, window


# ---- 1. precondition ---------------------------------------------------------------------
def test_probe_is_in_lock_step_with_the_reference_backend(run):
    _needs_oracle()
    record, _ = run
    with Simulator(ref_lib_path("contact_probe"), W, seed=cu.PROBE_SEED) as ref:
        for step in range(1, max(cu.STEPS) + 1):
            ref.step(1)
            if step in cu.STEPS:
                assert compare_columns(ref.dump_all(), record[step][0]) == [], step


# ---- 2. the definition -------------------------------------------------------------------
@pytest.mark.parametrize("poses", ["solver", "current"])
def test_equals_the_definition_through_the_reference_narrowphase(run, oracle, poses):
    lib, objects = oracle
    record, _ = run
    most = 0
    for step in cu.STEPS:
        dump, solver, current = record[step]
        want = cr.contact_ref(cu.worlds_of_dump(dump), objects, cu.ref_narrowphase(lib), K,
                              poses=poses)
        _same(solver if poses == "solver" else current, want, (poses, step))
        assert (want["status"] == cr.OK).all()
        most = max(most, int(want["count"].max()))
    assert most > K     # a world with more contacts than slots


# ---- 3. why solver poses are the default -------------------------------------------------
def test_a_body_at_rest_is_in_contact_in_every_step(run):
    """A dynamic body whose speed stays below 1e-3 over ten steps rests on
    something: at the solver poses it penetrates by about g h^2 = 9.8 * 0.01^2,
    far above rounding, so it is in a contact in each of the ten."""
    _, window = run
    assert len(window) == 10
    entity, _, response, _ = window[0]
    slow = np.ones(len(entity), bool)
    for e, velocity, _, _ in window:
        assert np.array_equal(e, entity)
        slow &= np.linalg.norm(velocity, axis=1) < 1e-3
    resting = entity[slow & (response == 0)]
    assert len(resting) >= 3, "no body came to rest"
    for step, (_, _, _, got) in zip(REST_WINDOW, window):
        assert (got["count"] <= UNCUT).all()
        touching = {tuple(e) for e in got["pairs"].reshape(-1, 2) if e[1] != -1}
        missing = [tuple(e) for e in resting if tuple(e) not in touching]
        assert not missing, (step, missing)


# ---- 4. plain == cooperative -------------------------------------------------------------
@pytest.mark.parametrize("sim,flags", [("contact_probe", 0), ("ball_pit", 0),
                                       ("escape_room_phys", 15), ("hideseek", 0)])
def test_plain_mapping_equals_the_cooperative_one(built, sim, flags):
    with Simulator(hip_lib_path(sim), W, seed=5, flags=flags) as s:
        queries = [(poses, s.contact_query(64, poses=poses),
                    s.contact_query(64, poses=poses, plain=True))
                   for poses in ("solver", "current")]
        found = 0
        for steps in (0, 5, 20):        # after 0, 5 and 25 steps
            s.step(steps)
            for poses, coop, plain in queries:
                got = _out(coop.compute())
                _same(_out(plain.compute()), got, (sim, poses, steps))
                assert (got["status"] == cr.OK).all()
                found += int(got["count"].sum())
        assert found > 0
        s.sync()


# ---- 5. K --------------------------------------------------------------------------------
def test_a_small_k_keeps_the_count_and_the_first_contacts(built):
    with _probe() as s:
        s.step(12)
        small, large = s.contact_query(3), s.contact_query(64)
        a, b = _out(small.compute()), _out(large.compute())
        assert np.array_equal(a["count"], b["count"]) and a["count"].max() > 64
        assert ((a["count"] > 0) & (a["count"] < 3)).any()
        for name in NAMES[2:]:
            assert np.array_equal(a[name], b[name][:, :3]), name
        behind = np.arange(3)[None, :] >= a["count"][:, None]
        assert (a["pairs"][behind] == -1).all() and (a["points"][behind] == 0).all()
        assert (a["num_points"][behind] == 0).all() and (a["normal"][behind] == 0).all()
        assert (a["pairs"][~behind] != -1).all()


# ---- 6. select ---------------------------------------------------------------------------
def test_select_owned_and_as_a_device_tensor(built):
    torch = _torch()
    pick = (np.arange(W) % 3 != 1).astype(np.int32)
    with _probe() as s:
        s.step(12)
        everything = _out(s.contact_query(K).compute())
        owned = s.contact_query(K, select=True)
        _same(_out(owned.compute()), everything, "every world selected at creation")
        owned.selects().copy_(torch.from_numpy(pick).cuda())
        source = torch.from_numpy(np.stack([pick, 1 - pick], 1).copy()).cuda()     # records of 8
        torch.cuda.synchronize()
        given = s.contact_query(K, select=source)
        with pytest.raises(RuntimeError, match="owns no select buffer"):
            given.selects()
        for q in (owned, given):
            got = _out(q.compute())
            off = pick == 0
            assert (got["status"][off] == cr.SKIPPED).all() and (got["count"][off] == 0).all()
            assert (got["pairs"][off] == -1).all() and (got["points"][off] == 0).all()
            assert (got["num_points"][off] == 0).all() and (got["normal"][off] == 0).all()
            for name in NAMES:
                assert np.array_equal(got[name][~off], everything[name][~off]), name
        assert everything["count"][pick == 0].sum() > 0


# ---- 7. before the first step ------------------------------------------------------------
def test_compute_before_the_first_step(built, oracle):
    """No body has been stepped: every stored q is zero and every body is taken
    where it is, so solver poses == current poses == the definition."""
    lib, objects = oracle
    with _probe() as s:
        solver, current = s.contact_query(K), s.contact_query(K, poses="current")
        got = _out(solver.compute())
        assert (got["status"] == cr.OK).all()
        _same(got, _out(current.compute()), "nothing stepped yet")
        dump = s.dump_all()
        assert not dump["Body.PreSolvePositional"][0].any()
        want = cr.contact_ref(cu.worlds_of_dump(dump), objects, cu.ref_narrowphase(lib), K,
                              poses="solver")
        _same(got, want, "before the first step")
        s.sync()        # (no sticky error)
        s.step(1)


# ---- 8. a world write between steps ------------------------------------------------------
def test_a_world_write_shows_at_current_poses_without_a_step(built, oracle):
    lib, objects = oracle
    with _probe() as s, s.world_write("Body", ["Body.Position"], max_rows=16) as write:
        torch = _torch()
        s.step(3)
        current = s.contact_query(K, poses="current")
        before = _out(current.compute())
        dump = s.dump_all()
        rows, counts = dump["Body.Position"]
        assert counts[0] == 16      # the first pen: plane, 4 walls, 11 cubes
        entity = dump["Body.Entity"][0].view(np.int32)[:16]
        mover, target = 15, 14      # its two highest cubes, still falling and apart
        pair = {tuple(entity[mover]), tuple(entity[target])}
        assert not any({tuple(p[0]), tuple(p[1])} == pair for p in before["pairs"][0])
        position = rows.view(np.float32).reshape(-1, 3)[:16].copy()
        position[mover] = position[target] + np.float32([0.2, 0.1, 0.3])
        slab = np.zeros((W, 16, 12), np.uint8)
        slab[0] = position.view(np.uint8).reshape(16, 12)
        take = np.zeros(W, np.int32)
        take[0] = 16
        write.tensor("Body.Position").copy_(torch.from_numpy(slab).cuda())
        write.take.copy_(torch.from_numpy(take).cuda())
        torch.cuda.synchronize()
        write.apply()
        got = _out(current.compute())
        assert any({tuple(p[0]), tuple(p[1])} == pair for p in got["pairs"][0])
        moved = s.dump_all()
        want = cr.contact_ref(cu.worlds_of_dump(moved), objects, cu.ref_narrowphase(lib), K,
                              poses="current")
        _same(got, want, "after the write")
        world = cu.worlds_of_dump(moved)[0]
        brute = cu.brute_force(world, objects, cu.ref_narrowphase(lib), "current")
        assert len(brute) == got["count"][0]
        assert [tuple(c[0]) + tuple(c[1]) for c in brute[:K]] == \
            [tuple(p.reshape(-1)) for p in got["pairs"][0, :len(brute)]]
        for name in NAMES:
            assert np.array_equal(got[name][1:], before[name][1:]), name


# ---- 9. the step stage -------------------------------------------------------------------
def test_every_step_against_a_twin_that_computes_on_demand(built):
    torch = _torch()
    rt = runtime_lib()
    STEPS = 6
    with _probe() as s, _probe() as twin, _probe() as never:
        names_without = [k["name"] for k in s.profile(1)]
        assert names_without == [k["name"] for k in never.profile(1)]
        assert LAUNCH not in names_without
        q, t_q = s.contact_query(K), twin.contact_query(K)
        gather = s.entity_gather(q.handle_source(), ["Position"])
        t_gather = twin.entity_gather(t_q.handle_source(), ["Position"])
        # made, not set: the launch list is still that of a simulator without one
        assert [k["name"] for k in s.profile(1)] == names_without
        twin.step(2)        # (a profile advances its simulator by the profiled step)
        q.every_step()
        gather.every_step()
        ring = torch.full((STEPS, W), 99, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert rt.mwhip_set_output_ring(s.hip_exec(), q.buffer_ptr("count"), ring.data_ptr(),
                                        W * 4, STEPS, RING_ON_STEP) == 0
        s.step_async(STEPS)
        trail = np.zeros((STEPS, W), np.int32)
        for k in range(STEPS):
            twin.step(1)
            want = _out(t_q.compute())
            t_gather.compute()
            trail[k] = want["count"]
        s.sync()
        assert np.array_equal(ring.cpu().numpy(), trail)
        assert trail.max() > 0 and not np.array_equal(trail[0], trail[-1])
        _same(_out(q), want, "the last replay")
        got_pos = gather.tensor("Position", np.float32).cpu().numpy()
        want_pos = t_gather.tensor("Position", np.float32).cpu().numpy()
        assert np.array_equal(got_pos.view(np.int32), want_pos.view(np.int32))
        # ... which are the ref bodies' positions (handle 2 * slot is a contact's ref)
        dump = s.dump_all()
        where = {tuple(e): p for e, p in zip(
            dump["Body.Entity"][0].view(np.int32), dump["Body.Position"][0].view(np.float32))}
        refs = want["pairs"].reshape(-1, 2, 2)[:, 0]
        slots = np.flatnonzero(refs[:, 1] != -1)
        assert len(slots) > 10
        for slot in slots:
            assert np.array_equal(got_pos[2 * slot], where[tuple(refs[slot])]), slot
        # exactly one launch more, behind the step's own and in front of the gather
        during = [k["name"] for k in s.profile(1)]
        assert during.count(LAUNCH) == 1
        at = during.index(LAUNCH)
        assert during[at + 1] == "gather:gather" and during[at + 2] == "ring:ring.out", during
        assert [n for n in during if n not in (LAUNCH, "gather:gather", "ring:ring.out")] == \
            names_without
        # carried replays: as many as the twin's, which has no step query
        for sim in (s, twin):
            sim.step_async(1)
            sim.sync()
        before = (s.broadphase_stats(), twin.broadphase_stats())
        for sim in (s, twin):
            sim.step_async(8)
            sim.sync()
        after = (s.broadphase_stats(), twin.broadphase_stats())
        carried = [a["carried_replays"] - b["carried_replays"] for a, b in zip(after, before)]
        assert carried[0] == carried[1], (before, after)
        assert rt.mwhip_set_output_ring(s.hip_exec(), q.buffer_ptr("count"), None, 0, 0,
                                        RING_ON_STEP) == 0
        gather.close()
        q.close()       # destroying a set query unsets it
        assert [k["name"] for k in s.profile(1)] == names_without


# ---- 10. snapshots -----------------------------------------------------------------------
def test_save_step_restore_compute(built):
    with _probe() as s, s.snapshot() as snap:
        s.step(12)
        queries = [s.contact_query(K), s.contact_query(K, poses="current")]
        at_save = [_out(q.compute()) for q in queries]
        snap.save()
        s.step(7)
        later = [_out(q.compute()) for q in queries]
        assert any(not np.array_equal(a["points"], b["points"]) for a, b in zip(at_save, later))
        snap.restore()
        for q, kept in zip(queries, later):
            _same(_out(q), kept, "derived state: not restored")
        for q, want in zip(queries, at_save):
            _same(_out(q.compute()), want, "restored and computed")


# ---- 11. refusals ------------------------------------------------------------------------
@pytest.mark.parametrize("sim", ["cartpole", "broadphase_only"])
def test_a_simulator_without_a_rigid_body_step_has_no_kernel(built, sim):
    with Simulator(hip_lib_path(sim), 4) as s:
        with pytest.raises(RuntimeError, match=r"-> -2.*registered no contact kernel"):
            s.contact_query(4, poses="current")
        assert s._contact_queries == []


def test_tgs_has_current_poses_only(built):
    with Simulator(hip_lib_path("tgs_drop"), W, seed=5) as s:
        with pytest.raises(RuntimeError, match=r"-> -2.*this simulator has no solver poses"):
            s.contact_query(8)
        coop = s.contact_query(8, poses="current")
        plain = s.contact_query(8, poses="current", plain=True)
        s.step(10)
        got = _out(coop.compute())
        _same(_out(plain.compute()), got, "tgs_drop")
        assert (got["status"] == cr.OK).all() and got["count"].sum() > 0
        s.sync()


def test_creation_limits_and_the_fifth_step_query(built):
    rt = runtime_lib()
    with _probe() as s:
        exec_ = s.hip_exec()
        out = C.c_uint64(77)

        def create(*fields):
            desc = ContactsDesc(*fields)
            return rt.mwhip_contacts_create(exec_, C.byref(desc), C.byref(out))

        assert create(0, 0, 0, 0) == -2 and "max_contacts is 0" in rt.mwhip_last_error().decode()
        assert create(2**27, 0, 0, 0) == -2 and "handles" in rt.mwhip_last_error().decode()
        assert create(4, 4, 0, 0) == -2 and "unknown flags" in rt.mwhip_last_error().decode()
        assert rt.mwhip_contacts_create(exec_, None, C.byref(out)) == -2
        assert out.value == 77
        status_ptr = s.contact_query(1).buffer_ptr("status")
        with pytest.raises(RuntimeError, match=r"-> -2.*multiples of 4"):
            s.contact_query(4, select=(status_ptr + 2, 4, 0))
        with pytest.raises(RuntimeError, match=r"-> -2.*do not fit a record"):
            s.contact_query(4, select=(status_ptr, 4, 4))
        with pytest.raises(ValueError):
            s.contact_query(4, poses="resting")

        before = [k["name"] for k in s.profile(1)]
        queries = [s.contact_query(2) for _ in range(5)]
        for q in queries[:4]:
            q.every_step()
        assert [k["name"] for k in s.profile(1)].count(LAUNCH) == 1
        with pytest.raises(RuntimeError, match=r"-> -2.*at most 4"):
            queries[4].every_step()
        queries[0].close()      # destroy unsets
        queries[4].every_step()
        s.step(2)
        assert all((_out(q)["status"] == cr.OK).all() for q in queries[1:])
        _same(_out(queries[1]), _out(queries[4]), "four plans in one launch")
        for q in queries[1:]:
            q.close()
        assert [k["name"] for k in s.profile(1)] == before
        assert s._contact_queries != [] and len(s._contact_queries) == 1


def test_a_handle_of_another_executor_is_refused(built):
    rt = runtime_lib()
    with _probe(3) as s, _probe(3) as other:
        q = s.contact_query(4)
        foreign = other.hip_exec()
        for call in (lambda: rt.mwhip_contacts_compute(foreign, q.handle),
                     lambda: rt.mwhip_contacts_compute_async(foreign, q.handle),
                     lambda: rt.mwhip_set_step_contacts(foreign, q.handle, 1),
                     lambda: rt.mwhip_set_step_contacts(foreign, q.handle, 0)):
            assert call() == -3
            assert "contact query %d is not one of this executor's" % q.handle in \
                rt.mwhip_last_error().decode()
        nbytes = C.c_uint64(5)
        assert rt.mwhip_contacts_buffer(foreign, q.handle, 1, C.byref(nbytes)) is None
        assert nbytes.value == 5
        rt.mwhip_contacts_destroy(foreign, q.handle)    # (not its own: nothing happens)
        assert LAUNCH not in [k["name"] for k in other.profile(1)]
        q.compute()
        assert rt.mwhip_contacts_buffer(s.hip_exec(), q.handle, 2, C.byref(nbytes)) is not None
        assert nbytes.value == 3 * 4
        # the select buffer of a query that owns none
        assert rt.mwhip_contacts_buffer(s.hip_exec(), q.handle, 0, C.byref(nbytes)) is None
        handle = q.handle
        q.close()
        assert rt.mwhip_contacts_compute(s.hip_exec(), handle) == -3   # destroyed
