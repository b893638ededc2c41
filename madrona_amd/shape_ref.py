"""Shape queries in numpy: the definition that mwhip_shapes_* (include/mwhip.h,
csrc/shape_query.hip, include/madrona/phys_impl/shape_query.inl)
is tested against, with the narrowphase injected as contact_ref.py does it.

Worlds and objects are contact_ref's: a world is a dict of arrays over its
bodies, the rows of the rigid-body archetypes in the step's iteration order (k =
0 .. n - 1), `objects[o]` lists the primitives of object o.

A query is F bundles of G shapes; shape s = f * G + g is shape g of bundle f, and
all shapes of a bundle lie in one world.  A shape is an object id, a position, a
rotation (w, x, y, z) and a scale, and an Entity (gen, id) to exclude.

What is tested: every body k of the shape's world whose entity is not the
excluded one (gen and id both), Static ones included, at its CURRENT pose, and of
it every primitive pair c = shapePrim * body_num_prims + bodyPrim.  The shape is
`a`; the two primitives are then ordered by type (a's <= b's), as
narrowphase::setupPair does.  The pair is a hit iff the primitives' world boxes
(AABB::applyTRS in float32) intersect and
    narrowphase(a, b) -> None | (ref_is_a, num_points, normal[3], points[4][4])
returns a manifold of at least one point, a and b being dicts with "prim",
"position", "rotation", "scale" and "body" (the shape's is -1) after the
ordering.  It raises Unsupported for a primitive pair no path supports.
ref_is_a only counts for a hull-hull pair; a plane is always the reference, and
so is b of any pair with a sphere.  shape_is_ref is 1 where that reference side
is the shape.

Order: ascending (k, c).  Point slots >= num_points are zero.
"""
from __future__ import annotations

import numpy as np

from .contact_ref import (HULL, PLANE, SPHERE, STATIC, Unsupported, apply_trs,  # noqa: F401
                          boxes_intersect)

OK, SKIPPED, BAD_WORLD, BAD_SHAPE, UNSORTED, UNSUPPORTED = 0, -1, -2, -3, -4, -5
NONE = (-1, -1)                         # Entity::none() as (gen, id) in int32


def shape_hits(world, objects, narrowphase, object_id, position, rotation, scale,
               exclude=NONE):
    """The hits of one shape in one world, uncapped, in order: a list of
    (entity[2], shape_is_ref, num_points, normal[3], points[4][4]).  Raises
    Unsupported."""
    n = len(world["object_id"])
    entity = np.asarray(world["entity"]).reshape(n, 2)
    position = np.asarray(position, np.float32)
    rotation = np.asarray(rotation, np.float32)
    scale = np.asarray(scale, np.float32)
    shape_prims = objects[int(object_id)]
    shape_boxes = [apply_trs(p["aabb"], position, rotation, scale) for p in shape_prims]
    shape = {"body": -1, "position": position, "rotation": rotation, "scale": scale}
    out = []
    for k in range(n):
        if int(entity[k, 0]) == int(exclude[0]) and int(entity[k, 1]) == int(exclude[1]):
            continue
        b_position = np.asarray(world["position"][k], np.float32)
        b_rotation = np.asarray(world["rotation"][k], np.float32)
        b_scale = np.asarray(world["scale"][k], np.float32)
        body = {"body": k, "position": b_position, "rotation": b_rotation, "scale": b_scale}
        body_prims = objects[int(world["object_id"][k])]
        body_boxes = [apply_trs(p["aabb"], b_position, b_rotation, b_scale) for p in body_prims]
        for s_idx, s_prim in enumerate(shape_prims):
            for b_idx, b_prim in enumerate(body_prims):
                if not boxes_intersect(shape_boxes[s_idx], body_boxes[b_idx]):
                    continue
                a = dict(shape, prim=s_prim)
                b = dict(body, prim=b_prim)
                if s_prim["type"] > b_prim["type"]:
                    a, b = b, a
                found = narrowphase(a, b)
                if found is None:
                    continue
                ref_is_a, num_points, normal, points = found
                if num_points < 1:
                    continue
                if a["prim"]["type"] != HULL or b["prim"]["type"] != HULL:
                    ref_is_a = False        # the plane; b of a sphere's pair
                ref = a if ref_is_a else b
                pts = np.zeros((4, 4), np.float32)
                pts[:num_points] = np.asarray(points, np.float32).reshape(4, 4)[:num_points]
                out.append((entity[k].copy(), 1 if ref["body"] == -1 else 0, int(num_points),
                            np.asarray(normal, np.float32).copy(), pts))
    return out


def _finite(*arrays) -> bool:
    return all(np.isfinite(np.asarray(a, np.float32)).all() for a in arrays)


def shape_ref(worlds, objects, narrowphase, shapes_per_bundle: int, max_hits: int, object_id,
              position, rotation, scale, world=None, bundles_per_world: int = 0, count=None,
              exclude=None, num_objects=None, unsorted: bool = False):
    """What a compute leaves: dict of status int32 [S], count int32 [S], hits
    int32 [S, K, 2], shape_is_ref int32 [S, K], num_points int32 [S, K], normal
    float32 [S, K, 3], points float32 [S, K, 4, 4].  worlds: a list of world
    dicts; object_id [S], position [S, 3], rotation [S, 4], scale [S, 3]; world:
    int32 [F] (unless bundles_per_world > 0); count: None or int32 [W], only with
    bundles_per_world > 0; exclude: None or int32 [S, 2]; num_objects: how many
    objects the manager holds (default: len(objects)); unsorted: a rigid-body
    table waits for its world sort.  Checks in the order world, count, then per
    shape."""
    G, K = int(shapes_per_bundle), int(max_hits)
    S = len(object_id)
    assert G >= 1 and K >= 1 and S % G == 0
    assert count is None or bundles_per_world > 0
    F, W = S // G, len(worlds)
    num_objects = len(objects) if num_objects is None else int(num_objects)
    out = {"status": np.zeros(S, np.int32), "count": np.zeros(S, np.int32),
           "hits": np.full((S, K, 2), -1, np.int32),
           "shape_is_ref": np.zeros((S, K), np.int32),
           "num_points": np.zeros((S, K), np.int32),
           "normal": np.zeros((S, K, 3), np.float32),
           "points": np.zeros((S, K, 4, 4), np.float32)}
    for f in range(F):
        w = f // bundles_per_world if bundles_per_world > 0 else int(world[f])
        head = OK
        if w < 0 or w >= W:
            head = BAD_WORLD
        elif count is not None and f % bundles_per_world >= int(count[w]):
            head = SKIPPED
        elif unsorted:
            head = UNSORTED
        for s in range(f * G, (f + 1) * G):
            if head != OK:
                out["status"][s] = head
                continue
            obj = int(object_id[s])
            if not _finite(position[s], rotation[s], scale[s]) or obj < 0 or obj >= num_objects:
                out["status"][s] = BAD_SHAPE
                continue
            try:
                hits = shape_hits(worlds[w], objects, narrowphase, obj, position[s], rotation[s],
                                  scale[s], NONE if exclude is None else exclude[s])
            except Unsupported:
                out["status"][s] = UNSUPPORTED
                continue
            out["count"][s] = len(hits)
            for k, (entity, is_ref, num_points, normal, points) in enumerate(hits[:K]):
                out["hits"][s, k] = entity
                out["shape_is_ref"][s, k] = is_ref
                out["num_points"][s, k] = num_points
                out["normal"][s, k] = normal
                out["points"][s, k] = points
    return out
