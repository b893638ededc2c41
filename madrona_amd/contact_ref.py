"""Contact queries in numpy: the definition that mwhip_contacts_* (include/mwhip.h,
csrc/contact_query.hip, include/madrona/phys_impl/contact_query.inl, DESIGN.md
§36) is tested against, with the narrowphase injected.

A world is a dict of arrays over its bodies, the rows of the rigid-body
archetypes in the step's iteration order (k = 0 .. n - 1):
    entity      int32 [n, 2]    (gen, id)
    position    float32 [n, 3]
    rotation    float32 [n, 4]  (w, x, y, z)
    scale       float32 [n, 3]
    object_id   int32 [n]
    response    int32 [n]       (ResponseType: STATIC == 2)
    presolve    float32 [n, 7]  xpbd::PreSolvePositional (x, then q as w, x, y, z);
                                only read with poses="solver"
`objects[o]` lists the primitives of object o, each a dict with "type" (SPHERE,
HULL or PLANE, the raw CollisionPrimitive::Type values) and "aabb" (float32 [6]:
pMin, pMax in object space, ObjectManager::primitiveAABBs).

Which pairs: every k_lo < k_hi that is not Static-Static, and of it every
primitive pair c = aPrim * b_num_prims + bPrim, where body a is the one with the
LOWER ENTITY ID.  The two primitives are then ordered by type (a's <= b's), as
narrowphase::setupPair does.  The pair is a contact iff the primitives' world
boxes (AABB::applyTRS in float32) intersect and
    narrowphase(a, b) -> None | (ref_is_a, num_points, normal[3], points[4][4])
returns a manifold of at least one point, a and b being dicts with "prim",
"position", "rotation", "scale" after the ordering.  It raises Unsupported for a
primitive pair no path supports.  ref_is_a only counts for a hull-hull pair; a
plane is always the reference, and so is b of any pair with a sphere.

Order: ascending (k_lo, k_hi, c).  Point slots >= num_points are zero.
"""
from __future__ import annotations

import numpy as np

SPHERE, HULL, PLANE = 1, 2, 4           # CollisionPrimitive::Type
STATIC = 2                              # ResponseType::Static
OK, SKIPPED, UNSORTED, UNSUPPORTED = 0, -1, -2, -3

_F = np.float32


class Unsupported(Exception):
    """narrowphase(): no path supports this primitive pair"""


def _rot_scale_columns(q, s):
    """math.hpp rotScaleColumns (Mat3x3::fromRS), float32, operation by operation"""
    w, x, y, z = (_F(v) for v in q)
    s0, s1, s2 = (_F(v) for v in s)
    x2, y2, z2 = x * x, y * y, z * z
    xz, xy, yz = x * z, x * y, y * z
    wx, wy, wz = w * x, w * y, w * z
    d0, d1, d2 = _F(2) * s0, _F(2) * s1, _F(2) * s2
    return ((s0 - d0 * (y2 + z2), d0 * (xy + wz), d0 * (xz - wy)),
            (d1 * (xy - wz), s1 - d1 * (x2 + z2), d1 * (yz + wx)),
            (d2 * (xz + wy), d2 * (yz - wx), s2 - d2 * (x2 + y2)))


def apply_trs(aabb, position, rotation, scale):
    """math::AABB::applyTRS in float32: (pMin[3], pMax[3])"""
    with np.errstate(all="ignore"):
        cols = _rot_scale_columns(rotation, scale)
        lo, hi = [], []
        for i in range(3):
            mn = mx = _F(position[i])
            for j in range(3):
                e = cols[j][i] * _F(aabb[j])
                f = cols[j][i] * _F(aabb[3 + j])
                if e < f:
                    mn, mx = mn + e, mx + f
                else:
                    mn, mx = mn + f, mx + e
            lo.append(mn)
            hi.append(mx)
    return lo, hi


def boxes_intersect(a, b) -> bool:
    """math::AABB::intersects: overlapping or exactly touching"""
    (a_lo, a_hi), (b_lo, b_hi) = a, b
    for i in range(3):
        if a_hi[i] < b_lo[i] or a_lo[i] > b_hi[i]:
            return False
    return True


def body_pose(world, k: int, poses: str):
    """(position, rotation) of body k in the mode `poses`"""
    if poses == "solver":
        solved = np.asarray(world["presolve"][k], np.float32)
        # q exactly zero: never stepped since it was created
        if np.any(solved[3:7] != 0):
            return solved[0:3], solved[3:7]
    return (np.asarray(world["position"][k], np.float32),
            np.asarray(world["rotation"][k], np.float32))


def world_contacts(world, objects, narrowphase, poses: str = "solver"):
    """The contacts of one world, uncapped, in order: a list of (ref_entity[2],
    alt_entity[2], num_points, normal[3], points[4][4]).  Raises Unsupported."""
    n = len(world["object_id"])
    entity = np.asarray(world["entity"]).reshape(n, 2)
    # (a primitive's world box depends on its body alone: made once)
    bodies = []
    for k in range(n):
        position, rotation = body_pose(world, k, poses)
        scale = np.asarray(world["scale"][k], np.float32)
        prims = objects[int(world["object_id"][k])]
        bodies.append({"body": k, "position": position, "rotation": rotation, "scale": scale,
                       "prims": prims,
                       "boxes": [apply_trs(p["aabb"], position, rotation, scale)
                                 for p in prims]})
    out = []
    for k_lo in range(n):
        for k_hi in range(k_lo + 1, n):
            if world["response"][k_lo] == STATIC and world["response"][k_hi] == STATIC:
                continue
            k_a, k_b = (k_lo, k_hi) if entity[k_lo, 1] < entity[k_hi, 1] else (k_hi, k_lo)
            sides = (bodies[k_a], bodies[k_b])
            for a_idx, a_prim in enumerate(sides[0]["prims"]):
                for b_idx, b_prim in enumerate(sides[1]["prims"]):
                    # (the test is symmetric: no need to order the boxes)
                    if not boxes_intersect(sides[0]["boxes"][a_idx], sides[1]["boxes"][b_idx]):
                        continue
                    a = dict(sides[0], prim=a_prim)
                    b = dict(sides[1], prim=b_prim)
                    if a_prim["type"] > b_prim["type"]:
                        a, b = b, a
                    found = narrowphase(a, b)
                    if found is None:
                        continue
                    ref_is_a, num_points, normal, points = found
                    if num_points < 1:
                        continue
                    if a["prim"]["type"] != HULL or b["prim"]["type"] != HULL:
                        ref_is_a = False        # the plane; b of a sphere's pair
                    ref, alt = (a, b) if ref_is_a else (b, a)
                    pts = np.zeros((4, 4), np.float32)
                    pts[:num_points] = np.asarray(points, np.float32).reshape(4, 4)[:num_points]
                    out.append((entity[ref["body"]].copy(), entity[alt["body"]].copy(),
                                int(num_points), np.asarray(normal, np.float32).copy(), pts))
    return out


def contact_ref(worlds, objects, narrowphase, max_contacts: int, select=None,
                poses: str = "solver", unsorted: bool = False):
    """What a compute leaves: dict of status int32 [W], count int32 [W], pairs
    int32 [W, K, 2, 2], num_points int32 [W, K], normal float32 [W, K, 3], points
    float32 [W, K, 4, 4].  worlds: a list of world dicts; select: None or int32
    [W]; unsorted: a rigid-body table waits for its world sort."""
    W, K = len(worlds), int(max_contacts)
    assert K >= 1 and poses in ("solver", "current")
    out = {"status": np.zeros(W, np.int32), "count": np.zeros(W, np.int32),
           "pairs": np.full((W, K, 2, 2), -1, np.int32),
           "num_points": np.zeros((W, K), np.int32),
           "normal": np.zeros((W, K, 3), np.float32),
           "points": np.zeros((W, K, 4, 4), np.float32)}
    for w, world in enumerate(worlds):
        if select is not None and int(select[w]) == 0:
            out["status"][w] = SKIPPED
            continue
        if unsorted:
            out["status"][w] = UNSORTED
            continue
        try:
            contacts = world_contacts(world, objects, narrowphase, poses)
        except Unsupported:
            out["status"][w] = UNSUPPORTED
            continue
        out["count"][w] = len(contacts)
        for k, (ref, alt, num_points, normal, points) in enumerate(contacts[:K]):
            out["pairs"][w, k, 0] = ref
            out["pairs"][w, k, 1] = alt
            out["num_points"][w, k] = num_points
            out["normal"][w, k] = normal
            out["points"][w, k] = points
    return out
