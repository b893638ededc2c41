"""GPU: ONE step launch that serves two objects of a kind whose wavefront item
counts differ (1 and 4: at least 3), for each of the seven step-batched kinds: world
views, world writes, world reduces, entity gathers, entity scatters, ray queries
and box queries.  The kernel has to find, for every work item of the launch, the
object it belongs to and its number there; with two objects of different sizes
the second object's items are numbered behind the first's.  Both orders of
setting are run.  4 worlds.

The yardstick is the object alone: after one step with both set, each object's
buffers equal, word for word, what the same object leaves after compute() on the
same state (the recomputing kinds run behind the step's nodes: compute() on the
state the step left), or what a twin simulator's object leaves after apply()
followed by the same step (writes and scatters run in front of them)."""
import numpy as np
import pytest

from madrona_amd import ray_ref
from madrona_amd.simlib import Simulator, hip_lib_path

pytestmark = pytest.mark.gpu

WORLDS = 4
POISON = 0x4D


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _sort_stress():
    return Simulator(hip_lib_path("sort_stress"), WORLDS, seed=7)


def _broadphase():
    return Simulator(hip_lib_path("broadphase_only"), WORLDS, seed=3, flags=1)


def _set(tensor, values):
    """writes a device tensor and WAITS (the executor's stream is non-blocking)"""
    torch = _torch()
    tensor.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(tensor.device))
    torch.cuda.synchronize()


def _read(tensors):
    _torch().cuda.synchronize()
    return [t.cpu().numpy().copy() for t in tensors]


def _poison(tensors):
    for t in tensors:
        t.view(_torch().uint8).fill_(POISON)
    _torch().cuda.synchronize()


def _workgroups(sim, name):
    """workgroups of the ONE launch called `name` in a step"""
    found = [k["workgroups"] for k in sim.profile(1) if k["name"] == name]
    assert len(found) == 1, (name, found)
    return found[0]


def _items_are_four_and_one(sim, objects, launch, like_small):
    """The premise, from the launch's grid (a workgroup per 4 work items).  The
    small object and three more of its shape fit ONE workgroup: 1 item each.  The
    big one alone fits one workgroup and needs a second with the small one: 4."""
    big, small = objects
    assert len(like_small) == 3
    for obj in objects:
        obj.every_step(False)
    for obj in [small] + like_small:
        obj.every_step()
    assert _workgroups(sim, launch) == 1, (launch, "four of the small one")
    for obj in [small] + like_small:
        obj.every_step(False)
    big.every_step()
    assert _workgroups(sim, launch) == 1, (launch, "the big one alone")
    small.every_step()
    assert _workgroups(sim, launch) == 2, (launch, "both")


def _ordered(pair, big_first):
    return pair if big_first else pair[::-1]


def _step_equals_compute(sim, objects, outputs, launch, big_first, like_small):
    """Both set (in the order asked for), one step; then each alone.  like_small:
    three more objects of the small one's shape, for the premise."""
    for obj in _ordered(objects, big_first):
        obj.every_step()
    for obj in objects:
        _poison(outputs(obj))
    sim.step(1)
    stepped = [_read(outputs(obj)) for obj in objects]
    for obj in objects:
        obj.every_step(False)
    for obj, by_step in zip(objects, stepped):
        _poison(outputs(obj))
        obj.compute()
        alone = _read(outputs(obj))
        for n, (a, b) in enumerate(zip(by_step, alone)):
            assert a.shape == b.shape and np.array_equal(a, b), (launch, big_first, n)
            assert not (b.view(np.uint8) == POISON).all(), (launch, "nothing was written", n)
    _items_are_four_and_one(sim, objects, launch, like_small)


def _handles(sim):
    """uint8 [200, 8] and [10, 8]: Item's Entity cells, world by world, zero
    padded (4 wavefronts of 64 handles, the first 40 once more; and 1)"""
    with sim.world_view("Item", ["Item.Entity"], max_rows=40) as view:
        view.compute()
        cells = view.tensor("Item.Entity").reshape(-1, 8).clone()
    return _torch().cat([cells, cells[:40]]).contiguous(), cells[3:13].contiguous()


def _views(sim, big_first):
    # teams of 64 lanes: a world per wavefront, 4 items; of 1 lane: 1 item
    objects = [sim.world_view("Item", ["Item.Vec3", "Item.Key"], max_rows=40),
               sim.world_view("Item", ["Item.Pair"], max_rows=1)]
    _step_equals_compute(
        sim, objects, lambda v: [v.tensor(c) for c in v.columns] + [v.counts], "view:view",
        big_first, [sim.world_view("Item", ["Item.Pair"], max_rows=1) for _ in range(3)])
    assert objects[0].counts.cpu().numpy().sum() > 0


def _reduces(sim, big_first):
    # 60 elements: teams of 64 lanes, 4 items; 1 element: 1 item
    objects = [sim.world_reduce("Item", [("Item.Wide", "sum", {"dtype": "u32"})]),
               sim.world_reduce("Item", [("Item.Key", "max")])]
    _step_equals_compute(
        sim, objects,
        lambda r: [r.tensor(i) for i in range(len(r.terms))] + [r.counts, r.alarm],
        "reduce:reduce", big_first,
        [sim.world_reduce("Item", [("Item.Key", "max")]) for _ in range(3)])
    assert objects[1].tensor(0).cpu().numpy().any()


def _gathers(sim, big_first):
    many, few = _handles(sim)
    # 200 handles: 4 items; 10: 1 item
    objects = [sim.entity_gather(many, ["Vec3", "Wide"]), sim.entity_gather(few, ["Key"])]
    _step_equals_compute(
        sim, objects,
        lambda g: [g.tensor(c) for c in g.components] + [g.archetypes, g.worlds],
        "gather:gather", big_first, [sim.entity_gather(few, ["Key"]) for _ in range(3)])
    assert (objects[0].archetypes.cpu().numpy() >= 0).any()
    assert (objects[1].archetypes.cpu().numpy() >= 0).any()


def _rays(sim, big_first):
    listed = [c[0] for c in sim.columns]
    pos, counts = sim.dump_column(listed.index("Sensor.Position"), 256)
    world = np.repeat(np.arange(WORLDS, dtype=np.int32), counts)
    origin = pos.view(np.float32).reshape(-1, 3)
    assert len(world) >= 2
    directions = ray_ref.fan_directions(False)      # [32, 3]
    # fans of 32 rays: a group of 32 lanes each, two to a wavefront: 4 items and 1
    objects = [sim.ray_query(8, 32), sim.ray_query(1, 32)]
    # (the sensors there are, once more from the first where they run out)
    for q, fans in zip(objects, (np.arange(8) % len(world), [len(world) - 1])):
        _set(q.worlds(), world[fans])
        _set(q.origins(), origin[fans])
        _set(q.directions(), np.tile(directions, (len(world[fans]), 1)))
        q.t_max().fill_(100.0)
    _torch().cuda.synchronize()
    _step_equals_compute(
        sim, objects, lambda q: [q.hit_t(), q.hits(), q.normals(), q.status()], "rays:rays",
        big_first, [sim.ray_query(1, 32) for _ in range(3)])
    assert (objects[0].status().cpu().numpy() == 1).any(), "no ray met anything"


def _boxes(sim, big_first):
    # bundles of up to 32 boxes: a group of 32 lanes each, two to a wavefront:
    # 8 bundles of 3 boxes are 4 items, 2 bundles of 1 box are 1 item
    objects = [sim.box_query(8, 3, 8), sim.box_query(2, 1, 8)]
    _set(objects[0].worlds(), np.array([0, 1, 2, 3, 0, 1, 2, 3], np.int32))
    _set(objects[1].worlds(), np.array([3, 2], np.int32))
    half = np.array([30.0, 8.0, 3.0] * 8, np.float32)[:, None] * np.ones((1, 3), np.float32)
    _set(objects[0].lo(), -half)
    _set(objects[0].hi(), half)
    _set(objects[1].lo(), np.full((2, 3), -30, np.float32))
    _set(objects[1].hi(), np.full((2, 3), 30, np.float32))
    _step_equals_compute(
        sim, objects, lambda q: [q.status(), q.counts(), q.hits()], "boxes:boxes", big_first,
        [sim.box_query(2, 1, 8) for _ in range(3)])
    assert objects[0].counts().cpu().numpy().max() > 0
    assert objects[1].counts().cpu().numpy().max() > 0


RECOMPUTED = {"view": (_sort_stress, _views), "reduce": (_sort_stress, _reduces),
              "gather": (_sort_stress, _gathers), "rays": (_broadphase, _rays),
              "boxes": (_broadphase, _boxes)}


@pytest.mark.parametrize("big_first", [True, False], ids=["big_first", "small_first"])
@pytest.mark.parametrize("kind", list(RECOMPUTED))
def test_one_step_launch_recomputes_two_objects_of_different_sizes(built, kind, big_first):
    make, run = RECOMPUTED[kind]
    with make() as sim:
        sim.step(2)
        run(sim, big_first)


# ---- writes and scatters: applied in front of the step's nodes -------------------------
def _same_state(sim, twin, what):
    got, want = sim.dump_all(), twin.dump_all()
    assert list(got) == list(want), what
    for name in want:
        for a, b in zip(got[name], want[name]):
            assert np.array_equal(a, b), (what, name)


def _make_writes(sim):
    # teams of 64 lanes: 4 items; of 1 lane: 1 item
    rng = np.random.default_rng(21)
    objects = [sim.world_write("Item", ["Item.Vec3", "Item.Pair"], max_rows=40),
               sim.world_write("Item", ["Item.Quad"], max_rows=1)]
    for w in objects:
        for column in w.columns:
            t = w.tensor(column)
            _set(t, rng.integers(0, 256, tuple(t.shape)).astype(np.uint8))
        _set(w.take, np.array([w.max_rows, 0, min(7, w.max_rows), w.max_rows], np.int32))
    # (three more of the small one's shape, taking no rows: for the premise)
    more = [sim.world_write("Item", [c], max_rows=1) for c in ("Item.Key", "Item.Half", "Item.Tag8")]
    return objects, (lambda w: [w.counts]), more


def _make_scatters(sim):
    # 200 handles: 4 items; 10: 1 item
    rng = np.random.default_rng(22)
    many, few = _handles(sim)
    objects = [sim.entity_scatter(many, ["Vec3", "Pair"]), sim.entity_scatter(few, ["Quad"])]
    for sc in objects:
        for name in sc.components:
            t = sc.tensor(name)
            _set(t, rng.integers(0, 256, tuple(t.shape)).astype(np.uint8))
        _set(sc.select, rng.integers(0, 3, sc.num_handles).astype(np.int32))
    # (three more of the small one's shape, selecting nothing: for the premise)
    more = [sim.entity_scatter(few, [c]) for c in ("Key", "Half", "Tag8")]
    return objects, (lambda sc: [sc.archetypes, sc.worlds, sc.written]), more


APPLIED = {"write": (_make_writes, "write:write"),
           "scatter": (_make_scatters, "scatter:scatter.write")}


@pytest.mark.parametrize("big_first", [True, False], ids=["big_first", "small_first"])
@pytest.mark.parametrize("kind", list(APPLIED))
def test_one_step_launch_applies_two_objects_of_different_sizes(built, kind, big_first):
    make, launch = APPLIED[kind]
    with _sort_stress() as sim, _sort_stress() as twin:
        sim.step(2)
        twin.step(2)
        _same_state(sim, twin, "before")
        objects, outputs, like_small = make(sim)
        twins, _, _ = make(twin)
        untouched = twin.dump_all()
        for obj in _ordered(objects, big_first):
            obj.every_step()
        for obj in objects + twins:
            _poison(outputs(obj))
        sim.step(1)
        for obj in _ordered(twins, big_first):
            obj.apply()
        applied = twin.dump_all()
        assert any(not np.array_equal(applied[name][0], untouched[name][0]) for name in applied), \
            "the applies changed nothing"
        twin.step(1)
        _same_state(sim, twin, (kind, "after the step"))
        for obj, alone in zip(objects, twins):
            for n, (a, b) in enumerate(zip(_read(outputs(obj)), _read(outputs(alone)))):
                assert a.shape == b.shape and np.array_equal(a, b), (kind, big_first, n)
                assert not (b.view(np.uint8) == POISON).all(), (kind, "nothing was written", n)
        _items_are_four_and_one(sim, objects, launch, like_small)
