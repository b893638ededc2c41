"""Helpers of the shape-query tests (test_shape_ref_cpu.py,
test_shape_query_gpu.py): the shapes the tests pose in a simulator's worlds,
generated from its dump by a seeded generator; the brute force over all bodies
with bounding spheres only; what a query computed as numpy arrays.  The
narrowphase, the objects and the worlds of a dump are contact_utils'."""
from __future__ import annotations

import numpy as np

import contact_utils as cu
from contact_utils import (PHYS_REF, PROBE_SEED, PROBE_WORLDS, STEPS, phys_ref,  # noqa: F401
                           probe_objects, worlds_of_dump)
from madrona_amd import contact_ref as cr
from madrona_amd import shape_ref as sr

MAX_HITS = 8            # the K of the GPU test: the plane shape in the crowded pen has more
SHAPE_SEED = 11
CUBE, PLANE, SPHERE = 0, 1, 2       # contact_probe's objects
CROWDED = 5             # contact_probe's crowded pen
NAMES = ("status", "count", "hits", "shape_is_ref", "num_points", "normal", "points")
UPRIGHT = (1.0, 0.0, 0.0, 0.0)


class Shapes:
    """S shapes as arrays: world int32 [S], object int32 [S], position float32
    [S, 3], rotation float32 [S, 4], scale float32 [S, 3], exclude int32 [S, 2];
    tag [S]: what the shape is for."""

    def __init__(self):
        self.rows, self.tag = [], []

    def add(self, tag, world, obj, position, rotation, scale, exclude=sr.NONE):
        self.rows.append((int(world), int(obj), np.asarray(position, np.float32),
                          np.asarray(rotation, np.float32), np.asarray(scale, np.float32),
                          np.asarray(exclude, np.int32)))
        self.tag.append(tag)

    def __len__(self):
        return len(self.rows)

    def _column(self, i, dtype, width):
        out = np.zeros((len(self.rows),) + ((width,) if width else ()), dtype)
        for s, row in enumerate(self.rows):
            out[s] = row[i]
        return out

    @property
    def world(self):
        return self._column(0, np.int32, 0)

    @property
    def object(self):
        return self._column(1, np.int32, 0)

    @property
    def position(self):
        return self._column(2, np.float32, 3)

    @property
    def rotation(self):
        return self._column(3, np.float32, 4)

    @property
    def scale(self):
        return self._column(4, np.float32, 3)

    @property
    def exclude(self):
        return self._column(5, np.int32, 2)

    def where(self, tag):
        return [s for s, t in enumerate(self.tag) if t == tag]

    def subset(self, picks):
        out = Shapes()
        for s in picks:
            out.rows.append(self.rows[s])
            out.tag.append(self.tag[s])
        return out


def body_shapes(worlds, objects, seed=SHAPE_SEED, displaced=True, judged_only=False):
    """From every dynamic body: its own object, pose and scale with exclude =
    that body ("own": what it touches), and, if `displaced`, the same moved by a
    fraction of its size with the body excluded ("moved") and not excluded
    ("moved_all").  judged_only: nothing the reference's scalar narrowphase
    cannot judge -- a sphere is never posed where another sphere or a plane can
    reach the narrowphase, so its "moved_all" twin is left out, and all sphere
    shapes of worlds that hold a plane."""
    rng = np.random.default_rng(seed)
    shapes = Shapes()
    for w, world in enumerate(worlds):
        n = len(world["object_id"])
        types = [objects[int(o)][0]["type"] for o in world["object_id"]]
        for k in range(n):
            # (drawn for every body, so that a shape does not depend on the flags)
            direction = rng.uniform(-1, 1, 3).astype(np.float32)
            if int(world["response"][k]) != 0:
                continue
            sphere = types[k] == cr.SPHERE
            if sphere and judged_only and (cr.PLANE in types or types.count(cr.SPHERE) > 1):
                continue
            me = np.asarray(world["entity"][k], np.int32)
            pose = (world["object_id"][k], world["position"][k], world["rotation"][k],
                    world["scale"][k])
            shapes.add("own", w, *pose, me)
            if not displaced:
                continue
            moved = (np.asarray(world["position"][k], np.float32) +
                     np.float32(0.3) * direction * np.asarray(world["scale"][k], np.float32))
            shapes.add("moved", w, pose[0], moved, pose[2], pose[3], me)
            if not (sphere and judged_only):
                shapes.add("moved_all", w, pose[0], moved, pose[2], pose[3])
    return shapes


def probe_shapes(worlds, objects):
    """The fixture of the oracle comparison on sims/contact_probe (16 worlds):
    body_shapes(judged_only) and the posed shapes the issue names.  No pair the
    reference's scalar narrowphase cannot judge reaches the narrowphase."""
    shapes = body_shapes(worlds, objects, judged_only=True)
    tilt = np.float32([0.98, 0.1, 0.05, 0.12])
    tilt /= np.linalg.norm(tilt)
    for w in (0, 4, 8, 12):     # pens of half width 1.6: floor plane, four wall cubes
        shapes.add("floor", w, CUBE, (0.1, -0.2, 0.25), UPRIGHT, (0.8, 1.3, 0.6))
        shapes.add("floor", w, CUBE, (-0.4, 0.3, 0.3), tilt, (1.4, 0.7, 0.9))
        shapes.add("wall", w, CUBE, (-1.5, 0.2, 1.2), tilt, (0.9, 0.5, 1.1))
        shapes.add("wall", w, CUBE, (0.3, 1.45, 2.0), UPRIGHT, (0.6, 0.8, 0.7))
        shapes.add("air", w, CUBE, (0.0, 0.0, 60.0), UPRIGHT, (1.0, 1.0, 1.0))
    # a plane shape that cuts the crowded pen's lower layer; the pen's own plane
    # is excluded (plane-plane is no pair of the narrowphase)
    crowded = worlds[CROWDED]
    planes = np.flatnonzero(np.asarray(crowded["object_id"]) == PLANE)
    assert len(planes) == 1
    shapes.add("plane", CROWDED, PLANE, (0.0, 0.0, 0.45), UPRIGHT, (1.0, 1.0, 1.0),
               crowded["entity"][planes[0]])
    shapes.add("air", CROWDED, CUBE, (0.0, 0.0, 60.0), UPRIGHT, (1.0, 1.0, 1.0))
    # a sphere shape on the slab of the worlds without a plane, away from the
    # world's own sphere (which stays within 2 of the middle)
    for w in (1, 9, 13):
        shapes.add("sphere", w, SPHERE, (3.0, -3.0, 1.15), UPRIGHT, (1.0, 1.0, 1.0))
        shapes.add("sphere", w, SPHERE, (-3.2, 3.0, 1.0), UPRIGHT, (1.0, 1.0, 1.0))
    # the world without bodies, the statics-only world
    shapes.add("empty", 3, CUBE, (0.0, 0.0, 0.3), UPRIGHT, (1.0, 1.0, 1.0))
    shapes.add("empty", 7, SPHERE, (0.0, 0.0, 0.3), UPRIGHT, (1.0, 1.0, 1.0))
    shapes.add("statics", 2, CUBE, (0.5, 0.1, 0.4), tilt, (1.2, 0.8, 0.9))
    return shapes


def bundled(shapes, shapes_per_bundle):
    """`shapes` ordered by world (stably), each world's padded with cubes high
    in the air to a multiple of shapes_per_bundle: bundles of one world each"""
    out = Shapes()
    for w in sorted({row[0] for row in shapes.rows}):
        for s, row in enumerate(shapes.rows):
            if row[0] == w:
                out.rows.append(row)
                out.tag.append(shapes.tag[s])
        while len(out) % shapes_per_bundle:
            out.add("air", w, CUBE, (0.0, 0.0, 90.0), UPRIGHT, (1.0, 1.0, 1.0))
    return out


def logging_narrowphase(narrowphase, log):
    """`narrowphase`, every call noted in `log` as (a body, b body, a type, b
    type, what it returned); the shape's body is -1"""
    def logged(a, b):
        found = narrowphase(a, b)
        log.append((a["body"], b["body"], a["prim"]["type"], b["prim"]["type"], found))
        return found
    return logged


def brute_force(world, objects, narrowphase, object_id, position, rotation, scale,
                exclude=sr.NONE):
    """Every body that is not excluded and whose bounding sphere meets the
    shape's, every primitive pair of the two, straight to the narrowphase: NO
    box test.  Same tuples, same order as shape_ref.shape_hits."""
    n = len(world["object_id"])
    entity = np.asarray(world["entity"]).reshape(n, 2)
    position = np.asarray(position, np.float32)
    rotation = np.asarray(rotation, np.float32)
    scale = np.asarray(scale, np.float32)
    posed = {"scale": [scale], "object_id": [int(object_id)]}
    shape_radius = cu._bounding_radius(posed, 0, objects)
    shape = {"body": -1, "position": position, "rotation": rotation, "scale": scale}
    out = []
    for k in range(n):
        if int(entity[k, 0]) == int(exclude[0]) and int(entity[k, 1]) == int(exclude[1]):
            continue
        b_position = np.asarray(world["position"][k], np.float32)
        apart = np.linalg.norm(position.astype(np.float64) - b_position.astype(np.float64))
        if apart > shape_radius + cu._bounding_radius(world, k, objects):
            continue
        body = {"body": k, "position": b_position,
                "rotation": np.asarray(world["rotation"][k], np.float32),
                "scale": np.asarray(world["scale"][k], np.float32)}
        for s_prim in objects[int(object_id)]:
            for b_prim in objects[int(world["object_id"][k])]:
                a, b = dict(shape, prim=s_prim), dict(body, prim=b_prim)
                if a["prim"]["type"] > b["prim"]["type"]:
                    a, b = b, a
                found = narrowphase(a, b)
                if found is None or found[1] < 1:
                    continue
                ref_is_a, num_points, normal, points = found
                if a["prim"]["type"] != cr.HULL or b["prim"]["type"] != cr.HULL:
                    ref_is_a = False
                ref = a if ref_is_a else b
                pts = np.zeros((4, 4), np.float32)
                pts[:num_points] = np.asarray(points, np.float32).reshape(4, 4)[:num_points]
                out.append((entity[k].copy(), 1 if ref["body"] == -1 else 0, int(num_points),
                            np.asarray(normal, np.float32).copy(), pts))
    return out


def same_hits(a, b) -> bool:
    """two lists of hit tuples, bit for bit"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if not (np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2] and
                np.array_equal(x[3].view(np.uint32), y[3].view(np.uint32)) and
                np.array_equal(x[4].view(np.uint32), y[4].view(np.uint32))):
            return False
    return True


def definition(worlds, objects, narrowphase, shapes, max_hits, shapes_per_bundle=1, **more):
    """shape_ref on `shapes`, a bundle per shape unless told otherwise"""
    world = shapes.world[::shapes_per_bundle]
    return sr.shape_ref(worlds, objects, narrowphase, shapes_per_bundle, max_hits, shapes.object,
                        shapes.position, shapes.rotation, shapes.scale, world=world,
                        exclude=shapes.exclude, **more)


def same(a, b, what, rows_a=None, rows_b=None):
    """two results (dicts of arrays over NAMES), bit for bit, order included;
    rows_*: the shapes of each to compare, all by default"""
    for name in NAMES:
        x, y = a[name], b[name]
        if rows_a is not None:
            x = x[rows_a]
        if rows_b is not None:
            y = y[rows_b]
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        bad = np.argwhere(x != y)
        assert bad.size == 0, (what, name, bad[:4].tolist())
