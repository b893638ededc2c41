"""CPU-only: madrona_amd/shape_ref.py, the definition of a shape query
(mwhip_shapes_*).  On synthetic input with a stand-in narrowphase:
order, the K cut, exclude, Static bodies, the statuses and their order, the
bundle layout, the fill behind the hits.  With the oracle built: the
reference-backend contact_probe simulator at steps 1, 3, 12, 40 -- the
definition, which tests the primitives' boxes first, against a brute force over
all bodies straight through the reference's narrowphase (ref_collide_pair), on
the shapes of tests/shape_utils.py, and the conditions that make
tests/test_shape_query_gpu.py non-vacuous."""
import os

import numpy as np
import pytest

import shape_utils as su
from conftest import ref_available
from madrona_amd import contact_ref as cr
from madrona_amd import shape_ref as sr
from madrona_amd.simlib import Simulator, ref_lib_path

UNIT = np.array([-.5, -.5, -.5, .5, .5, .5], np.float32)
OBJECTS = [
    [{"type": cr.HULL, "aabb": UNIT}],                                      # 0: a box
    [{"type": cr.HULL, "aabb": UNIT}, {"type": cr.SPHERE, "aabb": UNIT}],   # 1: two primitives
    [{"type": cr.PLANE, "aabb": np.array([-3e38, -3e38, -3e38, 3e38, 3e38, 0], np.float32)}],
]
ROW = [[0, 0, 0], [0.9, 0, 0], [1.8, 0, 0], [10, 0, 0]]


def _world(positions, ids, objects=None, responses=None):
    n = len(positions)
    return {
        "entity": np.stack([np.full(n, 3, np.int32), np.asarray(ids, np.int32)], 1).reshape(n, 2),
        "position": np.asarray(positions, np.float32).reshape(n, 3),
        "rotation": np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)),
        "scale": np.ones((n, 3), np.float32),
        "object_id": np.asarray(objects if objects is not None else [0] * n, np.int32),
        "response": np.asarray(responses if responses is not None else [0] * n, np.int32),
    }


def _touching(log=None):
    """Every pair whose boxes intersect touches: one point at a's position,
    normal = b - a, a the reference of a hull-hull pair iff it is the shape."""
    def narrowphase(a, b):
        if log is not None:
            log.append((a["body"], a["prim"]["type"], b["body"], b["prim"]["type"]))
        points = np.full((4, 4), 7.0, np.float32)       # (garbage behind num_points)
        points[0, :3] = a["position"]
        points[0, 3] = 0.25
        return a["body"] == -1, 1, b["position"] - a["position"], points
    return narrowphase


def _query(worlds, positions, world, K=4, G=1, objects=None, narrowphase=None, **more):
    S = len(positions)
    return sr.shape_ref(worlds, OBJECTS, narrowphase or _touching(), G, K,
                        objects if objects is not None else [0] * S,
                        np.asarray(positions, np.float32).reshape(S, 3),
                        np.tile(np.float32([1, 0, 0, 0]), (S, 1)), np.ones((S, 3), np.float32),
                        world=world, **more)


def test_order_counts_fill_and_which_side_is_the_reference():
    worlds = [_world(ROW, [5, 6, 7, 8])]
    out = _query(worlds, [[0.45, 0, 0], [30, 0, 0]], [0, 0])
    assert out["status"].tolist() == [sr.OK, sr.OK] and out["count"].tolist() == [2, 0]
    # ascending body k; the shape is a and, here, the reference
    assert out["hits"][0, :2].tolist() == [[3, 5], [3, 6]]
    assert out["shape_is_ref"][0].tolist() == [1, 1, 0, 0]
    assert (out["hits"][0, 2:] == -1).all() and (out["hits"][1] == -1).all()
    assert out["num_points"][0].tolist() == [1, 1, 0, 0]
    assert out["normal"][0, 0].tolist() == [np.float32(-0.45), 0, 0]
    assert out["points"][0, 0, 0].tolist() == [np.float32(0.45), 0, 0, 0.25]
    # point slots from num_points on are zero, whatever the narrowphase left there
    assert (out["points"][0, :, 1:] == 0).all() and (out["points"][0, 2:] == 0).all()
    assert (out["normal"][0, 2:] == 0).all() and (out["points"][1] == 0).all()


def test_count_is_not_capped_and_the_first_k_are_kept():
    worlds = [_world(ROW, [5, 6, 7, 8])]
    full = _query(worlds, [[0.9, 0, 0]], [0], K=4)
    cut = _query(worlds, [[0.9, 0, 0]], [0], K=2)
    assert full["count"].tolist() == [3] and cut["count"].tolist() == [3]
    assert cut["hits"].shape == (1, 2, 2)
    for name in su.NAMES[2:]:
        assert np.array_equal(cut[name][0], full[name][0, :2]), name


def test_static_bodies_are_tested_and_exclude_needs_gen_and_id():
    worlds = [_world(ROW, [5, 6, 7, 8], responses=[cr.STATIC] * 4)]
    assert _query(worlds, [[0.9, 0, 0]], [0])["count"].tolist() == [3]
    out = _query(worlds, [[0.9, 0, 0]] * 3, [0, 0, 0],
                 exclude=np.int32([[3, 6], [4, 6], [-1, -1]]))
    assert out["count"].tolist() == [2, 3, 3]
    assert out["hits"][0, :2, 1].tolist() == [5, 7]


def test_primitive_pairs_in_order_and_ordered_by_type():
    # the shape has object 1 (a hull and a sphere) and so has the body
    log = []
    out = _query([_world(ROW[:1], [9], objects=[1])], [[0.5, 0, 0]], [0], K=8, objects=[1],
                 narrowphase=_touching(log))
    assert out["count"].tolist() == [4]
    # c = shapePrim * 2 + bodyPrim; within a pair the sphere (type 1) comes first
    assert log == [(-1, cr.HULL, 0, cr.HULL), (0, cr.SPHERE, -1, cr.HULL),
                   (-1, cr.SPHERE, 0, cr.HULL), (-1, cr.SPHERE, 0, cr.SPHERE)]
    # b is the reference of every pair with a sphere: the shape in the second
    assert out["shape_is_ref"][0, :4].tolist() == [1, 1, 0, 0]


def test_a_plane_is_the_reference_whichever_side_it_is():
    body_plane = [_world([[0, 0, 0]], [2], objects=[2], responses=[cr.STATIC])]
    out = _query(body_plane, [[0, 0, 5], [0, 0, 0.2]], [0, 0])
    assert out["count"].tolist() == [0, 1] and out["shape_is_ref"][1, 0] == 0
    out = _query([_world([[0, 0, 0.2]], [4])], [[0, 0, 0]], [0], objects=[2])
    assert out["count"].tolist() == [1] and out["shape_is_ref"][0, 0] == 1


def test_statuses_in_the_order_world_count_shape():
    worlds = [_world(ROW, [5, 6, 7, 8]), _world([], [])]
    nan = float("nan")
    out = _query(worlds, [[0.9, 0, 0], [nan, 0, 0], [0.9, 0, 0], [0.9, 0, 0], [0.9, 0, 0]],
                 [0, 0, -1, 2, 1], objects=[0, 0, 0, 0, 7])
    assert out["status"].tolist() == [sr.OK, sr.BAD_SHAPE, sr.BAD_WORLD, sr.BAD_WORLD,
                                      sr.BAD_SHAPE]
    assert out["count"].tolist() == [3, 0, 0, 0, 0] and (out["hits"][1:] == -1).all()
    # an object past num_objects, and one below it
    assert _query(worlds, [[0.9, 0, 0]], [0], objects=[1], num_objects=1)["status"][0] == \
        sr.BAD_SHAPE
    assert _query(worlds, [[0.9, 0, 0]], [0], objects=[-1])["status"][0] == sr.BAD_SHAPE
    # bundles_per_world with count: two bundles of two shapes a world; a world
    # is checked before its count, a count before the shapes
    S = 8
    out = sr.shape_ref(worlds, OBJECTS, _touching(), 2, 2, [0] * S,
                       np.float32([[nan, 0, 0]] + [[0.9, 0, 0]] * (S - 1)),
                       np.tile(np.float32([1, 0, 0, 0]), (S, 1)), np.ones((S, 3), np.float32),
                       bundles_per_world=2, count=[1, 2])
    assert out["status"].tolist() == [sr.BAD_SHAPE, sr.OK, sr.SKIPPED, sr.SKIPPED, sr.OK, sr.OK,
                                      sr.OK, sr.OK]
    assert out["count"].tolist() == [0, 3, 0, 0, 0, 0, 0, 0]
    out = _query(worlds, [[0.9, 0, 0]], [0], unsorted=True)
    assert out["status"].tolist() == [sr.UNSORTED] and out["count"].tolist() == [0]

    def refuses(a, b):
        raise sr.Unsupported()
    out = _query(worlds, [[0.9, 0, 0], [50, 0, 0], [0, 0, 0]], [0, 0, 1], narrowphase=refuses)
    assert out["status"].tolist() == [sr.UNSUPPORTED, sr.OK, sr.OK]
    assert out["count"].tolist() == [0, 0, 0] and (out["hits"] == -1).all()


def test_the_helpers_are_contact_refs():
    assert sr.apply_trs is cr.apply_trs and sr.boxes_intersect is cr.boxes_intersect
    assert (sr.HULL, sr.PLANE, sr.SPHERE, sr.STATIC) == (cr.HULL, cr.PLANE, cr.SPHERE, cr.STATIC)
    assert sr.Unsupported is cr.Unsupported


# ---- the probe on the reference backend ----------------------------------------------

needs_oracle = pytest.mark.skipif(
    not (ref_available("contact_probe") and os.path.exists(su.PHYS_REF)),
    reason="oracle/_ref not built here (no reference tree)")


@pytest.fixture(scope="module")
def probe():
    """per compared step: the worlds of the reference-backend probe, the shapes
    posed in them and per shape the definition's hits with the pairs it sent to
    the narrowphase.  ref_narrowphase raising Unsupported fails here."""
    lib = su.phys_ref()
    objects = su.probe_objects(lib)
    steps = {}
    with Simulator(ref_lib_path("contact_probe"), su.PROBE_WORLDS, seed=su.PROBE_SEED) as sim:
        for step in range(1, max(su.STEPS) + 1):
            sim.step(1)
            if step in su.STEPS:
                worlds = su.worlds_of_dump(sim.dump_all())
                shapes = su.probe_shapes(worlds, objects)
                found = []
                for s, (w, obj, position, rotation, scale, exclude) in enumerate(shapes.rows):
                    calls = []
                    narrowphase = su.logging_narrowphase(su.cu.ref_narrowphase(lib), calls)
                    found.append((sr.shape_hits(worlds[w], objects, narrowphase, obj, position,
                                                rotation, scale, exclude), calls))
                steps[step] = (worlds, shapes, found)
    return lib, objects, steps


@needs_oracle
def test_definition_equals_brute_force_through_the_reference_narrowphase(probe):
    """The box test of the definition rejects no pair the narrowphase accepts."""
    lib, objects, steps = probe
    for step, (worlds, shapes, found) in steps.items():
        for s, (w, obj, position, rotation, scale, exclude) in enumerate(shapes.rows):
            brute = su.brute_force(worlds[w], objects, su.cu.ref_narrowphase(lib), obj, position,
                                   rotation, scale, exclude)
            assert su.same_hits(brute, found[s][0]), (step, s, shapes.tag[s], len(brute),
                                                      len(found[s][0]))


@needs_oracle
def test_shape_ref_lays_the_hits_out_as_the_list_says(probe):
    lib, objects, steps = probe
    worlds, shapes, found = steps[12]
    out = su.definition(worlds, objects, su.cu.ref_narrowphase(lib), shapes, su.MAX_HITS)
    assert (out["status"] == sr.OK).all()
    assert out["count"].tolist() == [len(hits) for hits, _ in found]
    for s, (hits, _) in enumerate(found):
        for k, (entity, is_ref, num_points, normal, points) in enumerate(hits[:su.MAX_HITS]):
            assert np.array_equal(out["hits"][s, k], entity)
            assert out["shape_is_ref"][s, k] == is_ref and out["num_points"][s, k] == num_points
            assert np.array_equal(out["points"][s, k], points)
        assert (out["hits"][s, len(hits):] == -1).all()


@needs_oracle
def test_probe_shapes_produce_every_kind_of_hit(probe):
    """What makes the GPU test non-vacuous, on the reference alone (the counts
    are in DESIGN.md §39)."""
    _, _, steps = probe
    kinds = {"face_shape_ref": 0, "face_body_ref": 0, "one_point": 0, "shape_on_plane4": 0,
             "sphere_shape_on_hull": 0, "plane_shape_on_hull": 0}
    most = 0
    empty_with_bodies = in_empty_world = exclude_drops = False
    for step, (worlds, shapes, found) in steps.items():
        for s, (hits, calls) in enumerate(found):
            w = shapes.rows[s][0]
            most = max(most, len(hits))
            if len(worlds[w]["object_id"]) and not hits:
                empty_with_bodies = True
            if not len(worlds[w]["object_id"]):
                in_empty_world = True
                assert not hits
            for a_body, b_body, a_type, b_type, result in calls:
                if result is None or result[1] < 1:
                    continue
                ref_is_a, num_points = result[0], result[1]
                shape_is_a = a_body == -1
                if (a_type, b_type) == (cr.HULL, cr.HULL):
                    if num_points == 1:
                        kinds["one_point"] += 1
                    elif ref_is_a == shape_is_a:
                        kinds["face_shape_ref"] += 1
                    else:
                        kinds["face_body_ref"] += 1
                elif (a_type, b_type) == (cr.HULL, cr.PLANE):
                    if shape_is_a and num_points == 4:
                        kinds["shape_on_plane4"] += 1
                    if not shape_is_a:
                        kinds["plane_shape_on_hull"] += 1
                elif (a_type, b_type) == (cr.SPHERE, cr.HULL) and shape_is_a:
                    kinds["sphere_shape_on_hull"] += 1
        # "moved" and "moved_all" are the same shape with and without exclude
        for s in shapes.where("moved"):
            if s + 1 < len(shapes) and shapes.tag[s + 1] == "moved_all":
                me = tuple(shapes.rows[s][5])
                with_me = found[s + 1][0]
                mine = [h for h in with_me if tuple(h[0]) == me]
                assert su.same_hits([h for h in with_me if tuple(h[0]) != me], found[s][0])
                if mine and len(found[s][0]) == len(with_me) - len(mine):
                    exclude_drops = True
    print("hit kinds over steps %s: %s; most hits of a shape %d" % (su.STEPS, kinds, most))
    assert all(n >= 1 for n in kinds.values()), kinds
    assert most > su.MAX_HITS       # a shape with more hits than the GPU test's K
    assert empty_with_bodies and in_empty_world and exclude_drops
