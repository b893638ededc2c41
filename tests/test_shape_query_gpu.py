"""Shape queries (mwhip_shapes_*, Simulator.shape_query) on the
device.  The yardsticks are not the code under test: madrona_amd/shape_ref.py
with the reference's own scalar narrowphase (ref_collide_pair of
oracle/_ref/libphys_ref.so) over the dumps of the contact_probe simulator (which
tests/test_contact_query_gpu.py shows to be in lock step with the reference
backend) on the shapes of tests/shape_utils.py; and the plain mapping -- the
generic single-lane routine, pair after pair -- for the cooperative one on
shapes the oracle cannot judge."""
import ctypes as C
import os

import numpy as np
import pytest

import shape_utils as su
from conftest import ref_available
from madrona_amd import shape_ref as sr
from madrona_amd.simlib import (RING_ON_STEP, ShapesDesc, Simulator, hip_lib_path, runtime_lib)

pytestmark = pytest.mark.gpu

W, K = su.PROBE_WORLDS, su.MAX_HITS
NUM_OBJECTS = 3         # contact_probe's: Cube, Plane, Sphere
LAUNCH = "shapes:shapes"


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _out(q):
    _torch().cuda.synchronize()
    return {"status": q.status().cpu().numpy(), "count": q.counts().cpu().numpy(),
            "hits": q.hits().cpu().numpy(), "shape_is_ref": q.shape_is_ref().cpu().numpy(),
            "num_points": q.num_points().cpu().numpy(), "normal": q.normals().cpu().numpy(),
            "points": q.points().cpu().numpy()}


def _fill(q, shapes, world=True, exclude=True):
    """the shapes into the query's owned inputs (a bundle's world is its first
    shape's)"""
    torch = _torch()
    def put(tensor, array):
        tensor.copy_(torch.from_numpy(np.ascontiguousarray(array)).cuda())
    put(q.objects(), shapes.object)
    put(q.positions(), shapes.position)
    put(q.rotations(), shapes.rotation)
    put(q.scales(), shapes.scale)
    if exclude:
        put(q.excludes(), shapes.exclude)
    if world:
        put(q.worlds(), shapes.world[::q.shapes_per_bundle])
    torch.cuda.synchronize()
    return q


def _query(sim, shapes, max_hits=K, G=1, num_objects=NUM_OBJECTS, plain=False):
    assert len(shapes) % G == 0
    return _fill(sim.shape_query(len(shapes) // G, G, max_hits, num_objects, plain=plain), shapes)


def _probe(worlds=W):
    return Simulator(hip_lib_path("contact_probe"), worlds, seed=su.PROBE_SEED)


def _needs_oracle():
    if not (ref_available("contact_probe") and os.path.exists(su.PHYS_REF)):
        pytest.skip("oracle/_ref not built here (no reference tree)")


@pytest.fixture(scope="module")
def oracle(built):
    _needs_oracle()
    lib = su.phys_ref()
    return lib, su.probe_objects(lib)


def _objects():
    """contact_probe's objects by type alone (no oracle needed: the boxes are
    only read by the definition)"""
    return [[{"type": sr.HULL}], [{"type": sr.PLANE}], [{"type": sr.SPHERE}]]


@pytest.fixture(scope="module")
def run(built):
    """The HIP probe at every compared step: its dump, the shapes posed in it
    and what the cooperative and the plain query computed for them."""
    record = {}
    with _probe() as sim:
        coop = plain = None
        for step in range(1, max(su.STEPS) + 1):
            sim.step(1)
            if step in su.STEPS:
                dump = sim.dump_all()
                shapes = su.probe_shapes(su.worlds_of_dump(dump), _objects())
                if coop is None:
                    coop = sim.shape_query(len(shapes), 1, K, NUM_OBJECTS)
                    plain = sim.shape_query(len(shapes), 1, K, NUM_OBJECTS, plain=True)
                record[step] = (dump, shapes, _out(_fill(coop, shapes).compute()),
                                _out(_fill(plain, shapes).compute()))
        sim.sync()      # (no sticky error)
    return record


# ---- 1. the definition -------------------------------------------------------------------
@pytest.mark.parametrize("mapping", ["cooperative", "plain"])
def test_equals_the_definition_through_the_reference_narrowphase(run, oracle, mapping):
    lib, objects = oracle
    most = 0
    for step in su.STEPS:
        dump, shapes, coop, plain = run[step]
        worlds = su.worlds_of_dump(dump)
        want = su.definition(worlds, objects, su.cu.ref_narrowphase(lib), shapes, K)
        su.same(coop if mapping == "cooperative" else plain, want, (mapping, step))
        assert (want["status"] == sr.OK).all()
        most = max(most, int(want["count"].max()))
        assert want["shape_is_ref"].sum() > 0 and (want["count"] == 0).any()
    assert most > K     # a shape with more hits than slots


# ---- 2. plain == cooperative, shapes the oracle cannot judge included --------------------
BODIES = {      # simulator: (flags, objects, tables of dynamic bodies that dump Entity and pose)
    "contact_probe": (0, 3, ("Body",)),
    "ball_pit": (0, 7, ("MovableObject",)),
    "escape_room_phys": (15, 6, ("Agent", "PhysicsEntity")),
    "hideseek": (0, 7, ("Agent", "MovableObject")),
    "tgs_drop": (0, 2, ("Body",)),
}


def _shapes_of_bodies(dump, tables, num_objects, worlds):
    """Every body of `tables` as a shape at its own pose with itself excluded,
    and moved by a third of a unit without; the object ids run through all the
    simulator's objects (spheres, planes and many-sided hulls among them), the
    scales through three."""
    rng = np.random.default_rng(su.SHAPE_SEED)
    scales = np.float32([[1, 1, 1], [0.7, 1.2, 0.9], [1.5, 1.5, 1.5]])
    shapes, n = su.Shapes(), 0
    for table in tables:
        entity, counts = dump[f"{table}.Entity"]
        entity = entity.view(np.int32).reshape(-1, 2)
        position = dump[f"{table}.Position"][0].view(np.float32).reshape(-1, 3)
        rotation = dump[f"{table}.Rotation"][0].view(np.float32).reshape(-1, 4)
        world = np.repeat(np.arange(worlds), counts[:worlds])
        for row in range(len(entity)):
            obj, scale = n % num_objects, scales[n % 3]
            n += 1
            moved = position[row] + rng.uniform(-0.33, 0.33, 3).astype(np.float32)
            shapes.add("own", world[row], obj, position[row], rotation[row], scale, entity[row])
            shapes.add("moved_all", world[row], obj, moved, rotation[row], scale)
    return shapes


@pytest.mark.parametrize("sim", list(BODIES))
def test_plain_mapping_equals_the_cooperative_one(built, sim):
    flags, num_objects, tables = BODIES[sim]
    worlds = 8
    with Simulator(hip_lib_path(sim), worlds, seed=5, flags=flags) as s:
        found = 0
        queries = None
        for steps in (0, 5, 20):        # after 0, 5 and 25 steps
            s.step(steps)
            shapes = _shapes_of_bodies(s.dump_all(), tables, num_objects, worlds)
            if queries is None:
                queries = [s.shape_query(len(shapes), 1, 6, num_objects, plain=p)
                           for p in (False, True)]
            got = _out(_fill(queries[0], shapes).compute())
            su.same(_out(_fill(queries[1], shapes).compute()), got, (sim, steps))
            assert np.isin(got["status"], (sr.OK, sr.UNSUPPORTED)).all()
            assert (got["count"][got["status"] != sr.OK] == 0).all()
            found += int(got["count"].sum())
        assert found > 0
        s.sync()


# ---- 3. bundles --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crowd(built):
    """130 shapes in the crowded pen after 12 steps, and what a bundle per shape
    computes for them"""
    with _probe() as s:
        s.step(12)
        worlds = su.worlds_of_dump(s.dump_all())
        everything = su.body_shapes(worlds, _objects())
        shapes = everything.subset([i for i in range(len(everything))
                                    if everything.rows[i][0] == su.CROWDED][:130])
        assert len(shapes) == 130
        alone = _out(_query(s, shapes).compute())
        assert alone["count"].sum() > 200 and (alone["status"] == sr.OK).all()
        yield s, shapes, alone


@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("plain", [False, True])
def test_bundles_of_edge_sizes_equal_the_same_shapes_unbundled(crowd, G, plain):
    s, shapes, alone = crowd
    padded = shapes.subset(range(len(shapes)))
    while len(padded) % G:
        padded.add("air", su.CROWDED, su.CUBE, (0, 0, 70), su.UPRIGHT, (1, 1, 1))
    with _query(s, padded, G=G, plain=plain) as q:
        got = _out(q.compute())
    rows = np.arange(len(shapes))
    su.same(got, alone, ("G", G, plain), rows_a=rows)
    assert (got["count"][len(shapes):] == 0).all() and (got["status"] == sr.OK).all()


@pytest.mark.parametrize("plain", [False, True])
def test_two_bundles_in_one_world_equal_the_two_computed_alone(crowd, plain):
    """Two wavefronts of one launch in the same world: each has its own slot of
    the executor's scratch."""
    s, shapes, alone = crowd
    both = shapes.subset(range(128))
    with _query(s, both, G=64, plain=plain) as q, \
            _query(s, shapes.subset(range(64)), G=64, plain=plain) as first, \
            _query(s, shapes.subset(range(64, 128)), G=64, plain=plain) as second:
        got = _out(q.compute())
        su.same(got, _out(first.compute()), "first", rows_a=np.arange(64))
        su.same(got, _out(second.compute()), "second", rows_a=np.arange(64, 128))
        su.same(got, alone, "unbundled", rows_b=np.arange(128))


# ---- 4. inputs ---------------------------------------------------------------------------
def test_bundles_per_world_with_count_and_sources(built, oracle):
    """world by rule with a per-world count; world and exclude as sources: a
    tensor, and a world view's slab of the Entity column with its counts."""
    torch = _torch()
    lib, objects = oracle
    R = 16
    with _probe() as s, s.world_view("Body", ["Body.Entity"], max_rows=R) as view:
        s.step(12)
        view.compute()
        dump = s.dump_all()
        worlds = su.worlds_of_dump(dump)
        # shape (w, r): body r of world w where it stands, without itself
        with s.shape_query(W * R, 1, K, NUM_OBJECTS, bundles_per_world=R, count=view.counts,
                           exclude=(view.buffer_ptr("Body.Entity"), 8, 0)) as q:
            with pytest.raises(RuntimeError, match="owns no world buffer"):
                q.worlds()
            with pytest.raises(RuntimeError, match="owns no exclude buffer"):
                q.excludes()
            shapes = su.Shapes()
            counts = np.zeros(W, np.int32)
            for w, world in enumerate(worlds):
                n = len(world["object_id"])
                counts[w] = n
                for r in range(R):
                    if r < n and world["object_id"][r] != su.PLANE:
                        shapes.add("own", w, world["object_id"][r], world["position"][r],
                                   world["rotation"][r], world["scale"][r], world["entity"][r])
                    else:
                        # (a plane is no shape to pose against cubes it holds
                        # up; rows past the count are skipped)
                        shapes.add("air", w, su.CUBE, (0, 0, 80), su.UPRIGHT, (1, 1, 1),
                                   world["entity"][r] if r < n else (0, 0))
            got = _out(_fill(q, shapes, world=False, exclude=False).compute())
            want = sr.shape_ref(worlds, objects, su.cu.ref_narrowphase(lib), 1, K, shapes.object,
                                shapes.position, shapes.rotation, shapes.scale,
                                bundles_per_world=R, count=counts, exclude=shapes.exclude)
            su.same(got, want, "rule, count and a view's slab")
            assert (got["status"] == sr.SKIPPED).sum() > R and got["count"].sum() > 20
            assert (got["status"][su.CROWDED * R:(su.CROWDED + 1) * R] == sr.OK).all()
        # the same through tensors: records of 12 bytes with the world in front,
        # records of 8 bytes
        picks = [i for i in range(len(shapes)) if got["status"][i] == sr.OK]
        sub = shapes.subset(picks)
        world_src = torch.from_numpy(np.stack(
            [sub.world, -np.ones(len(sub), np.int32), 7 * np.ones(len(sub), np.int32)],
            1).copy()).cuda()
        exclude_src = torch.from_numpy(sub.exclude.copy()).cuda()
        torch.cuda.synchronize()
        with s.shape_query(len(sub), 1, K, NUM_OBJECTS, world=world_src,
                           exclude=exclude_src) as given:
            su.same(_out(_fill(given, sub, world=False, exclude=False).compute()), got,
                    "tensor sources", rows_b=np.array(picks))


def test_statuses_next_to_good_shapes(built):
    with _probe() as s:
        s.step(12)
        worlds = su.worlds_of_dump(s.dump_all())
        good = su.bundled(su.probe_shapes(worlds, _objects()), 4)
        clean = _out(_query(s, good, G=4).compute())
        assert (clean["status"] == sr.OK).all()
        # creation state: object 0 at the identity in world 0, nothing excluded
        with s.shape_query(2, 2, K, NUM_OBJECTS) as fresh:
            assert fresh.objects().cpu().tolist() == [0] * 4
            assert fresh.rotations().cpu().tolist() == [[1, 0, 0, 0]] * 4
            assert fresh.scales().cpu().tolist() == [[1, 1, 1]] * 4
            assert fresh.positions().cpu().abs().sum() == 0
            assert fresh.excludes().cpu().tolist() == [[-1, -1]] * 4
            assert fresh.worlds().cpu().tolist() == [0, 0]
            for name in ("world", "exclude", "object", "position", "rotation", "scale", "status",
                         "count", "hits", "shape_is_ref", "num_points", "normal", "points"):
                assert fresh.buffer_ptr(name) % 256 == 0, name
            assert (_out(fresh.compute())["status"] == sr.OK).all()
        bad = good.subset(range(len(good)))
        nan, inf = np.float32("nan"), np.float32("inf")
        spoil = {1: (2, 0, nan), 6: (3, 2, nan), 11: (4, 1, inf), 13: (4, 0, -inf)}
        for row, (column, element, value) in spoil.items():
            fields = list(bad.rows[row])
            fields[column] = fields[column].copy()
            fields[column][element] = value
            bad.rows[row] = tuple(fields)
        for row, obj in ((17, NUM_OBJECTS), (22, -1), (23, 2**31 - 1)):
            bad.rows[row] = (bad.rows[row][0], obj) + bad.rows[row][2:]
        bad_worlds = {7: -1, 9: W, 10: -2**31}
        for bundle, w in bad_worlds.items():
            bad.rows[bundle * 4] = (w,) + bad.rows[bundle * 4][1:]
        # (a bad shape in a bundle of a bad world: the world is checked first)
        bad.rows[7 * 4 + 1] = (0, 99) + bad.rows[7 * 4 + 1][2:]
        got = _out(_query(s, bad, G=4).compute())
        want_status = np.zeros(len(bad), np.int32)
        for row in list(spoil) + [17, 22, 23]:
            want_status[row] = sr.BAD_SHAPE
        for bundle in bad_worlds:
            want_status[bundle * 4:bundle * 4 + 4] = sr.BAD_WORLD
        assert got["status"].tolist() == want_status.tolist()
        off = want_status != sr.OK
        assert (got["count"][off] == 0).all() and (got["hits"][off] == -1).all()
        assert (got["points"][off] == 0).all() and (got["normal"][off] == 0).all()
        assert (got["num_points"][off] == 0).all() and (got["shape_is_ref"][off] == 0).all()
        assert clean["count"][off].sum() > 0
        su.same(got, clean, "the good shapes", rows_a=~off, rows_b=~off)
        s.sync()        # (no sticky error)
        s.step(1)


APPEND_ONLY, COMPACT_ONLY = 1, 2     # contact_probe: a body more per world, unsorted; the sort


def test_a_body_table_that_waits_for_its_world_sort_gives_unsorted(built):
    """needsSort belongs to the table: while it is set no world has a row range,
    so every shape whose world and count are good is UNSORTED.  A bad world is
    found before that."""
    with _probe() as s:
        s.step(12)
        worlds = su.worlds_of_dump(s.dump_all())
        shapes = su.bundled(su.probe_shapes(worlds, _objects()), 4)
        shapes.rows[3 * 4] = (W,) + shapes.rows[3 * 4][1:]                  # bundle 3: no world
        shapes.rows[5 * 4 + 1] = shapes.rows[5 * 4 + 1][:1] + (NUM_OBJECTS,) + \
            shapes.rows[5 * 4 + 1][2:]                                      # a bad shape
        queries = [_query(s, shapes, G=4, plain=plain) for plain in (False, True)]
        clean = _out(queries[0].compute())
        assert clean["count"].sum() > 100 and (clean["status"] == sr.OK).sum() > len(shapes) - 6
        s.run_taskgraph(APPEND_ONLY)
        want = su.definition(worlds, _objects(), None, shapes, K, shapes_per_bundle=4,
                             num_objects=NUM_OBJECTS, unsorted=True)
        bad_world = np.zeros(len(shapes), bool)
        bad_world[3 * 4:4 * 4] = True
        assert (want["status"][bad_world] == sr.BAD_WORLD).all()
        assert (want["status"][~bad_world] == sr.UNSORTED).all()
        for q in queries:
            got = _out(q.compute())
            su.same(got, want, "unsorted")
            assert (got["count"] == 0).all() and (got["hits"] == -1).all()
            assert (got["points"] == 0).all() and (got["num_points"] == 0).all()
        s.sync()        # (no sticky error)
        # the sort it waited for: the new cube, far above everything, is hit by nothing
        s.run_taskgraph(COMPACT_ONLY)
        for q in queries:
            su.same(_out(q.compute()), clean, "sorted again")
        s.step(1)
        assert (_out(queries[0].compute())["status"] == clean["status"]).all()


# ---- 5. state ----------------------------------------------------------------------------
def test_compute_before_the_first_step_and_a_world_write_without_a_step(built, oracle):
    lib, objects = oracle
    torch = _torch()
    with _probe() as s, s.world_write("Body", ["Body.Position"], max_rows=16) as write:
        dump = s.dump_all()
        worlds = su.worlds_of_dump(dump)
        shapes = su.probe_shapes(worlds, objects)
        q = _query(s, shapes)
        got = _out(q.compute())
        su.same(got, su.definition(worlds, objects, su.cu.ref_narrowphase(lib), shapes, K),
                "before the first step")
        assert got["count"].sum() > 0
        s.sync()
        s.step(3)
        # a cube of the first pen is written into the "air" shape of that world
        dump = s.dump_all()
        air = [i for i in shapes.where("air") if shapes.rows[i][0] == 0][0]
        before = _out(q.compute())
        assert before["count"][air] == 0
        rows, counts = dump["Body.Position"]
        assert counts[0] == 16
        position = rows.view(np.float32).reshape(-1, 3)[:16].copy()
        position[15] = shapes.rows[air][2] + np.float32([0.2, 0.1, 0.3])
        slab = np.zeros((W, 16, 12), np.uint8)
        slab[0] = position.view(np.uint8).reshape(16, 12)
        take = np.zeros(W, np.int32)
        take[0] = 16
        write.tensor("Body.Position").copy_(torch.from_numpy(slab).cuda())
        write.take.copy_(torch.from_numpy(take).cuda())
        torch.cuda.synchronize()
        write.apply()
        got = _out(q.compute())
        entity = dump["Body.Entity"][0].view(np.int32).reshape(-1, 2)
        assert got["count"][air] == 1 and got["hits"][air, 0].tolist() == entity[15].tolist()
        want = su.definition(su.worlds_of_dump(s.dump_all()), objects,
                             su.cu.ref_narrowphase(lib), shapes, K)
        su.same(got, want, "after the write")


def test_save_step_restore_compute(built):
    with _probe() as s, s.snapshot() as snap:
        s.step(12)
        shapes = su.probe_shapes(su.worlds_of_dump(s.dump_all()), _objects())
        q = _query(s, shapes)
        at_save = _out(q.compute())
        snap.save()
        s.step(7)
        later = _out(q.compute())
        assert not np.array_equal(at_save["points"], later["points"])
        snap.restore()
        su.same(_out(q), later, "derived state: not restored")
        su.same(_out(q.compute()), at_save, "restored and computed")


# ---- 6. the step stage -------------------------------------------------------------------
def test_every_step_against_a_twin_that_computes_on_demand(built):
    torch = _torch()
    rt = runtime_lib()
    STEPS = 6
    with _probe() as s, _probe() as twin:
        names_without = [k["name"] for k in s.profile(1)]
        assert LAUNCH not in names_without
        twin.step(1)
        shapes = su.probe_shapes(su.worlds_of_dump(s.dump_all()), _objects())
        S = len(shapes)
        q, t_q = _query(s, shapes), _query(twin, shapes)
        contacts, t_contacts = s.contact_query(4), twin.contact_query(4)
        gather = s.entity_gather(q.handle_source(), ["Position"])
        t_gather = twin.entity_gather(t_q.handle_source(), ["Position"])
        # made, not set: the launch list is still that of a simulator without one
        assert [k["name"] for k in s.profile(1)] == names_without
        twin.step(1)        # (a profile advances its simulator by the profiled step)
        q.every_step()
        contacts.every_step()
        gather.every_step()
        ring = torch.full((STEPS, S), 99, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert rt.mwhip_set_output_ring(s.hip_exec(), q.buffer_ptr("count"), ring.data_ptr(),
                                        S * 4, STEPS, RING_ON_STEP) == 0
        s.step_async(STEPS)
        trail = np.zeros((STEPS, S), np.int32)
        for k in range(STEPS):
            twin.step(1)
            want = _out(t_q.compute())
            t_gather.compute()
            trail[k] = want["count"]
        s.sync()
        assert np.array_equal(ring.cpu().numpy(), trail)
        assert trail.max() > K and not np.array_equal(trail[0], trail[-1])
        su.same(_out(q), want, "the last replay")
        got_pos = gather.tensor("Position", np.float32).cpu().numpy()
        want_pos = t_gather.tensor("Position", np.float32).cpu().numpy()
        assert np.array_equal(got_pos.view(np.int32), want_pos.view(np.int32))
        # ... which are the positions of the bodies hit
        dump = s.dump_all()
        where = {tuple(e): p for e, p in zip(
            dump["Body.Entity"][0].view(np.int32).reshape(-1, 2),
            dump["Body.Position"][0].view(np.float32).reshape(-1, 3))}
        hits = want["hits"].reshape(-1, 2)
        slots = np.flatnonzero(hits[:, 1] != -1)
        assert len(slots) > 10
        for slot in slots:
            assert np.array_equal(got_pos[slot], where[tuple(hits[slot])]), slot
        # together with a step contact query: the same contacts as the twin's
        t_contacts.compute()
        torch.cuda.synchronize()
        assert np.array_equal(contacts.pairs().cpu().numpy(), t_contacts.pairs().cpu().numpy())
        # exactly one launch more, behind the contacts and in front of the gather
        during = [k["name"] for k in s.profile(1)]
        assert during.count(LAUNCH) == 1
        at = during.index(LAUNCH)
        assert during[at - 1] == "contacts:contacts" and during[at + 1] == "gather:gather"
        assert during[at + 2] == "ring:ring.out", during
        assert [n for n in during if n not in (LAUNCH, "contacts:contacts", "gather:gather",
                                               "ring:ring.out")] == names_without
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
        contacts.close()
        q.close()       # destroying a set query unsets it
        assert [k["name"] for k in s.profile(1)] == names_without


# ---- 7. refusals -------------------------------------------------------------------------
@pytest.mark.parametrize("sim", ["cartpole", "broadphase_only"])
def test_a_simulator_without_a_rigid_body_step_has_no_kernel(built, sim):
    with Simulator(hip_lib_path(sim), 4) as s:
        with pytest.raises(RuntimeError, match=r"-> -2.*registered no shape kernel"):
            s.shape_query(2, 1, 4, 1)
        assert s._shape_queries == []


def test_creation_limits_and_the_fifth_step_query(built):
    rt = runtime_lib()
    with _probe() as s:
        exec_ = s.hip_exec()
        out = C.c_uint64(77)

        def create(*fields):
            desc = ShapesDesc(*fields)
            return rt.mwhip_shapes_create(exec_, C.byref(desc), C.byref(out))

        for fields in ((0, 1, 1, 1, 0, 0), (1, 0, 1, 1, 0, 0), (1, 1, 0, 1, 0, 0),
                       (1, 1, 1, 0, 0, 0)):
            assert create(*fields) == -2, fields
            assert "bundles of" in rt.mwhip_last_error().decode()
        assert create(2**16, 2**15, 1, 1, 0, 0) == -2
        assert "handles" in rt.mwhip_last_error().decode()
        assert create(2**16, 2**8, 2**8, 1, 0, 0) == -2
        assert "handles" in rt.mwhip_last_error().decode()
        assert create(1, 1, 1, 1, 0, 2) == -2 and "unknown flags" in rt.mwhip_last_error().decode()
        assert rt.mwhip_shapes_create(exec_, None, C.byref(out)) == -2
        assert out.value == 77
        status_ptr = s.shape_query(1, 1, 1, 1).buffer_ptr("status")
        # (a kernel registered without scratch would leave every output unwritten)
        assert rt.mwhip_set_shape_kernel(exec_, status_ptr, 0) == -2
        assert "scratch_bytes_per_wavefront is 0" in rt.mwhip_last_error().decode()
        with pytest.raises(RuntimeError, match=r"-> -2.*multiples of 4"):
            s.shape_query(1, 1, 1, 1, world=(status_ptr + 2, 4, 0))
        with pytest.raises(RuntimeError, match=r"-> -2.*do not fit a record"):
            s.shape_query(1, 1, 1, 1, exclude=(status_ptr, 4, 0))
        with pytest.raises(RuntimeError, match=r"-> -2.*count source needs bundles_per_world"):
            s.shape_query(1, 1, 1, 1, count=(status_ptr, 4, 0))

        before = [k["name"] for k in s.profile(1)]
        shapes = su.probe_shapes(su.worlds_of_dump(s.dump_all()), _objects())
        queries = [_query(s, shapes) for _ in range(5)]
        for q in queries[:4]:
            q.every_step()
        assert [k["name"] for k in s.profile(1)].count(LAUNCH) == 1
        with pytest.raises(RuntimeError, match=r"-> -2.*at most 4"):
            queries[4].every_step()
        queries[0].close()      # destroy unsets
        queries[4].every_step()
        s.step(2)
        assert all((_out(q)["status"] == sr.OK).all() for q in queries[1:])
        for q in queries[2:]:
            su.same(_out(queries[1]), _out(q), "four plans in one launch")
        su.same(_out(queries[1]), _out(queries[1].compute()), "a step's and a compute's")
        for q in queries[1:]:
            q.close()
        assert [k["name"] for k in s.profile(1)] == before
        assert len(s._shape_queries) == 1


def test_a_handle_of_another_executor_is_refused(built):
    rt = runtime_lib()
    with _probe(3) as s, _probe(3) as other:
        q = s.shape_query(2, 2, 4, NUM_OBJECTS)
        foreign = other.hip_exec()
        for call in (lambda: rt.mwhip_shapes_compute(foreign, q.handle),
                     lambda: rt.mwhip_shapes_compute_async(foreign, q.handle),
                     lambda: rt.mwhip_set_step_shapes(foreign, q.handle, 1),
                     lambda: rt.mwhip_set_step_shapes(foreign, q.handle, 0)):
            assert call() == -3
            assert "shape query %d is not one of this executor's" % q.handle in \
                rt.mwhip_last_error().decode()
        nbytes = C.c_uint64(5)
        assert rt.mwhip_shapes_buffer(foreign, q.handle, 6, C.byref(nbytes)) is None
        assert nbytes.value == 5
        rt.mwhip_shapes_destroy(foreign, q.handle)      # (not its own: nothing happens)
        assert LAUNCH not in [k["name"] for k in other.profile(1)]
        q.compute()
        assert rt.mwhip_shapes_buffer(s.hip_exec(), q.handle, 7, C.byref(nbytes)) is not None
        assert nbytes.value == 4 * 4
        assert rt.mwhip_shapes_buffer(s.hip_exec(), q.handle, 13, C.byref(nbytes)) is None
        handle = q.handle
        q.close()
        assert rt.mwhip_shapes_compute(s.hip_exec(), handle) == -3      # destroyed
