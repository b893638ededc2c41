"""CPU-only: madrona_amd/contact_ref.py, the definition of a contact query
(mwhip_contacts_*).  On synthetic input with a stand-in
narrowphase: order, the K cut, the Static-Static skip, select, the fill behind
the contacts, the lower-entity-id rule, the poses.  With the oracle built: the
reference-backend contact_probe simulator at steps 1, 3, 12, 40 -- the
definition, which tests the primitives' boxes first, against a brute force over
all pairs straight through the reference's narrowphase (ref_collide_pair), and
the conditions that make tests/test_contact_query_gpu.py non-vacuous."""
import os

import numpy as np
import pytest

import contact_utils as cu
from conftest import ref_available
from madrona_amd import contact_ref as cr
from madrona_amd.simlib import Simulator, ref_lib_path

UNIT = np.array([-.5, -.5, -.5, .5, .5, .5], np.float32)
OBJECTS = [
    [{"type": cr.HULL, "aabb": UNIT}],                                      # 0: a box
    [{"type": cr.HULL, "aabb": UNIT}, {"type": cr.SPHERE, "aabb": UNIT}],   # 1: two primitives
    [{"type": cr.PLANE, "aabb": np.array([-3e38, -3e38, -3e38, 3e38, 3e38, 0], np.float32)}],
]


def _world(positions, ids, objects=None, responses=None, presolve=None):
    n = len(positions)
    world = {
        "entity": np.stack([np.zeros(n, np.int32), np.asarray(ids, np.int32)], 1),
        "position": np.asarray(positions, np.float32).reshape(n, 3),
        "rotation": np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)),
        "scale": np.ones((n, 3), np.float32),
        "object_id": np.asarray(objects if objects is not None else [0] * n, np.int32),
        "response": np.asarray(responses if responses is not None else [0] * n, np.int32),
    }
    if presolve is not None:
        world["presolve"] = np.asarray(presolve, np.float32).reshape(n, 7)
    return world


def _touching(log=None):
    """Every pair whose boxes intersect touches: one point at a's position,
    normal = b - a, a the reference of a hull-hull pair iff it is the lower body."""
    def narrowphase(a, b):
        if log is not None:
            log.append((a["body"], a["prim"]["type"], b["body"], b["prim"]["type"]))
        points = np.full((4, 4), 7.0, np.float32)       # (garbage behind num_points)
        points[0, :3] = a["position"]
        points[0, 3] = 0.25
        return a["body"] < b["body"], 1, b["position"] - a["position"], points
    return narrowphase


ROW = [[0, 0, 0], [0.9, 0, 0], [1.8, 0, 0], [10, 0, 0]]    # 0-1 and 1-2 meet, 3 is far


def test_order_counts_and_fill():
    out = cr.contact_ref([_world(ROW, [5, 6, 7, 8])], OBJECTS, _touching(), 4, poses="current")
    assert out["status"].tolist() == [cr.OK] and out["count"].tolist() == [2]
    # ascending (k_lo, k_hi); the lower body is a and, here, the reference
    assert out["pairs"][0, :2, :, 1].tolist() == [[5, 6], [6, 7]]
    assert (out["pairs"][0, 2:] == -1).all()
    assert out["num_points"][0].tolist() == [1, 1, 0, 0]
    assert out["normal"][0, 0].tolist() == [np.float32(0.9), 0, 0]
    assert out["points"][0, 0, 0].tolist() == [0, 0, 0, 0.25]
    # point slots from num_points on are zero, whatever the narrowphase left there
    assert (out["points"][0, :, 1:] == 0).all() and (out["points"][0, 2:] == 0).all()
    assert (out["normal"][0, 2:] == 0).all()


def test_count_is_not_capped_and_the_first_k_are_kept():
    world = _world(ROW, [5, 6, 7, 8])
    full = cr.contact_ref([world], OBJECTS, _touching(), 4, poses="current")
    cut = cr.contact_ref([world], OBJECTS, _touching(), 1, poses="current")
    assert cut["count"].tolist() == [2] and cut["pairs"].shape == (1, 1, 2, 2)
    assert np.array_equal(cut["pairs"][0, 0], full["pairs"][0, 0])
    assert np.array_equal(cut["points"][0, 0], full["points"][0, 0])


def test_static_static_pairs_are_skipped_before_the_narrowphase():
    log = []
    out = cr.contact_ref([_world(ROW, [5, 6, 7, 8], responses=[cr.STATIC, cr.STATIC, 0, 0])],
                         OBJECTS, _touching(log), 4, poses="current")
    assert out["count"].tolist() == [1]
    assert [(a, b) for a, _, b, _ in log] == [(1, 2)]
    # a kinematic body (1) is not static
    out = cr.contact_ref([_world(ROW, [5, 6, 7, 8], responses=[cr.STATIC, 1, 0, 0])],
                         OBJECTS, _touching(), 4, poses="current")
    assert out["count"].tolist() == [2]


def test_boxes_that_do_not_intersect_never_reach_the_narrowphase():
    log = []
    cr.contact_ref([_world(ROW, [5, 6, 7, 8])], OBJECTS, _touching(log), 4, poses="current")
    assert [(a, b) for a, _, b, _ in log] == [(0, 1), (1, 2)]
    # exactly touching boxes intersect (AABB::intersects)
    log.clear()
    cr.contact_ref([_world([[0, 0, 0], [1, 0, 0]], [1, 2])], OBJECTS, _touching(log), 4,
                   poses="current")
    assert len(log) == 1


def test_the_body_of_lower_entity_id_is_a():
    # rows in the order of ids 9, 3: the second row is a
    log = []
    out = cr.contact_ref([_world(ROW[:2], [9, 3])], OBJECTS, _touching(log), 2, poses="current")
    assert [(a, b) for a, _, b, _ in log] == [(1, 0)]
    # ... and `a` is not the lower body, so the stand-in names b the reference
    assert out["pairs"][0, 0, :, 1].tolist() == [9, 3]
    assert out["normal"][0, 0].tolist() == [np.float32(-0.9), 0, 0]


def test_primitive_pairs_in_order_and_ordered_by_type():
    # body 0 (id 1) has object 1: a hull and a sphere; body 1 (id 2) likewise
    log = []
    out = cr.contact_ref([_world(ROW[:2], [1, 2], objects=[1, 1])], OBJECTS, _touching(log), 8,
                         poses="current")
    assert out["count"].tolist() == [4]
    # c = aPrim * 2 + bPrim; within a pair the sphere (type 1) comes first
    assert log == [(0, cr.HULL, 1, cr.HULL), (1, cr.SPHERE, 0, cr.HULL),
                   (0, cr.SPHERE, 1, cr.HULL), (0, cr.SPHERE, 1, cr.SPHERE)]
    # b is the reference of every pair with a sphere
    assert out["pairs"][0, :4, 0, 1].tolist() == [1, 1, 2, 2]


def test_a_plane_is_the_reference_and_meets_everything_above_and_below():
    out = cr.contact_ref([_world([[0, 0, 5], [0, 0, 0]], [1, 2], objects=[0, 2],
                                 responses=[0, cr.STATIC])], OBJECTS, _touching(), 2,
                         poses="current")
    assert out["count"].tolist() == [0]     # the box is above the plane's box
    out = cr.contact_ref([_world([[0, 0, 0.2], [0, 0, 0]], [1, 2], objects=[0, 2],
                                 responses=[0, cr.STATIC])], OBJECTS, _touching(), 2,
                         poses="current")
    assert out["count"].tolist() == [1] and out["pairs"][0, 0, :, 1].tolist() == [2, 1]


def test_select_and_the_other_statuses():
    worlds = [_world(ROW, [5, 6, 7, 8]), _world(ROW, [5, 6, 7, 8]), _world([], [])]
    out = cr.contact_ref(worlds, OBJECTS, _touching(), 2, select=[1, 0, 1], poses="current")
    assert out["status"].tolist() == [cr.OK, cr.SKIPPED, cr.OK]
    assert out["count"].tolist() == [2, 0, 0]
    assert (out["pairs"][1:] == -1).all() and (out["points"][1:] == 0).all()
    out = cr.contact_ref(worlds, OBJECTS, _touching(), 2, select=[1, 0, 1], poses="current",
                         unsorted=True)
    assert out["status"].tolist() == [cr.UNSORTED, cr.SKIPPED, cr.UNSORTED]
    assert out["count"].tolist() == [0, 0, 0]

    def refuses(a, b):
        raise cr.Unsupported()
    out = cr.contact_ref(worlds, OBJECTS, refuses, 2, poses="current")
    assert out["status"].tolist() == [cr.UNSUPPORTED, cr.UNSUPPORTED, cr.OK]
    assert out["count"].tolist() == [0, 0, 0] and (out["pairs"] == -1).all()


def test_solver_poses_and_the_zero_quaternion_rule():
    # body 1 was solved 5 m away; body 2 has never been stepped (q == 0)
    presolve = [[0, 0, 0, 1, 0, 0, 0], [5, 0, 0, 1, 0, 0, 0], [99, 99, 99, 0, 0, 0, 0]]
    world = _world(ROW[:3], [5, 6, 7], presolve=presolve)
    now = cr.contact_ref([world], OBJECTS, _touching(), 4, poses="current")
    assert now["pairs"][0, :2, :, 1].tolist() == [[5, 6], [6, 7]]
    solved = cr.contact_ref([world], OBJECTS, _touching(), 4, poses="solver")
    assert solved["count"].tolist() == [0]
    presolve[1][0] = 0.9
    solved = cr.contact_ref([_world(ROW[:3], [5, 6, 7], presolve=presolve)], OBJECTS,
                            _touching(), 4, poses="solver")
    assert solved["pairs"][0, :2, :, 1].tolist() == [[5, 6], [6, 7]]


def test_apply_trs_is_the_headers():
    """AABB::applyTRS of a rotated, scaled box, in float32 (Arvo's method)"""
    s = np.float32(np.sqrt(0.5))
    lo, hi = cr.apply_trs(UNIT, [1, 2, 3], [s, 0, 0, s], [2, 1, 1])      # 90 degrees about z
    assert np.allclose(lo, [0.5, 1, 2.5], atol=1e-6) and np.allclose(hi, [1.5, 3, 3.5], atol=1e-6)
    assert all(isinstance(v, np.float32) for v in lo + hi)


# ---- the probe on the reference backend ----------------------------------------------

needs_oracle = pytest.mark.skipif(
    not (ref_available("contact_probe") and os.path.exists(cu.PHYS_REF)),
    reason="oracle/_ref not built here (no reference tree)")


@pytest.fixture(scope="module")
def probe():
    """per compared step: the worlds of the reference-backend probe, and per
    world the definition's contacts at the current poses with the pairs it sent
    to the narrowphase"""
    lib = cu.phys_ref()
    objects = cu.probe_objects(lib)
    steps = {}
    with Simulator(ref_lib_path("contact_probe"), cu.PROBE_WORLDS, seed=cu.PROBE_SEED) as sim:
        for step in range(1, max(cu.STEPS) + 1):
            sim.step(1)
            if step in cu.STEPS:
                worlds = cu.worlds_of_dump(sim.dump_all())
                found = []
                for world in worlds:
                    calls = []
                    contacts = cr.world_contacts(world, objects, cu.ref_narrowphase(lib, calls),
                                                 "current")
                    found.append((contacts, calls))
                steps[step] = (worlds, found)
    return lib, objects, steps


@needs_oracle
def test_probe_worlds_are_the_kinds_the_issue_names(probe):
    _, _, steps = probe
    worlds, _ = steps[1]
    sizes = [len(w["object_id"]) for w in worlds]
    assert sizes[5] >= 70 and sizes[3] == 0 and sizes[2] > 0
    assert all((w["response"] == cr.STATIC).all() for w in worlds[2::4] if len(w["response"]))
    for w in worlds[1::4]:
        if len(w["object_id"]) and w is not worlds[5]:
            # one sphere, no plane: no sphere-plane and no sphere-sphere pair
            assert (w["object_id"] == 2).sum() == 1 and (w["object_id"] == 1).sum() == 0


@needs_oracle
def test_definition_equals_brute_force_through_the_reference_narrowphase(probe):
    """The box test of the definition rejects no pair the narrowphase accepts."""
    lib, objects, steps = probe
    for step, (worlds, found) in steps.items():
        for w, world in enumerate(worlds):
            brute = cu.brute_force(world, objects, cu.ref_narrowphase(lib), "current")
            assert cu.same_contacts(brute, found[w][0]), (step, w, len(brute), len(found[w][0]))


@needs_oracle
def test_probe_produces_every_kind_of_contact(probe):
    """What makes the GPU test non-vacuous, on the reference alone (the counts
    are in DESIGN.md §36)."""
    _, _, steps = probe
    kinds = {"face_a": 0, "face_b": 0, "one_point": 0, "plane4": 0, "sphere_hull": 0}
    most, most_sent, empty_with_bodies = 0, 0, False
    for step, (worlds, found) in steps.items():
        for w, (contacts, calls) in enumerate(found):
            most = max(most, len(contacts))
            most_sent = max(most_sent, len(calls))
            if len(worlds[w]["object_id"]) and not contacts:
                empty_with_bodies = True
            for types, out in calls:
                if out[0] == 0:
                    continue
                if types == (cr.HULL, cr.HULL):
                    if out[2] == 1:
                        kinds["one_point"] += 1
                    else:
                        kinds["face_a" if out[1] == 1 else "face_b"] += 1
                elif types == (cr.HULL, cr.PLANE) and out[2] == 4:
                    kinds["plane4"] += 1
                elif types == (cr.SPHERE, cr.HULL):
                    kinds["sphere_hull"] += 1
    print("contact kinds over steps %s: %s; most contacts in a world %d, most pairs sent %d"
          % (cu.STEPS, kinds, most, most_sent))
    assert all(n >= 1 for n in kinds.values()), kinds
    assert most > cu.MAX_CONTACTS       # a world with more contacts than the GPU test's K
    assert most_sent > 64               # ... and more than one chunk of survivors
    assert empty_with_bodies
