"""Box queries in numpy: the definition that mwhip_boxes_* (include/mwhip.h,
csrc/box_query.hip, include/madrona/phys_impl/box_query.inl)
computes on the device, and the yardstick of its tests.  The per-world
enumeration is injected, as ray_ref.py injects the tracer: this file defines
everything AROUND it -- bundles, sources and strides, bundles_per_world and
counts, every status and the order of the checks, K truncation, the output
conventions -- and `enumerate_world(world, p_min, p_max) -> [(gen, id), ...] |
None` says which entities PhysicsSystem::findEntitiesWithinAABB reports for
the box, in its order (on the device: the leaves of the world's tree in
traversal order whose own box overlaps the query and whose hull does); None
for a world whose tree no broadphase pass has built yet.

B = F * G boxes, F bundles of G >= 1 boxes that share a world and a centre;
box b = f * G + g is box g of bundle f:

    pMin = centre[f] + lo[b],  pMax = centre[f] + hi[b]        (float32)

A SOURCE is (buf, record_bytes, first_byte), as in ray_ref.py.

    world[f]    int32.  bundles_per_world > 0 replaces it: f // bundles_per_world.
    count[w]    optional int32 per world, only with bundles_per_world > 0:
                bundle f with f % bundles_per_world >= count[world] is SKIPPED.
    centre[f]   3 float32.
    lo[b], hi[b]  3 float32 each.

Checked in this order, and nothing behind a failed check is read:

    BAD_WORLD (-2)  world not in [0, num_worlds)
    SKIPPED   (-1)  by the count rule
    BAD_BOX   (-3)  a non-finite component of the centre; then, per box, a
                    non-finite component of lo or hi, a non-finite sum, or
                    pMin > pMax on an axis
    OK (0)

    count[b]    int32: how many entities are reported, NOT capped by K; 0 on
                anything but OK
    hits[b][k]  uint32 [2] (gen, id), k < K: the first min(count, K) entities
                in report order, Entity::none() = (0xFFFFFFFF, 0xFFFFFFFF)
                behind them

Also here: an enumeration over axis-aligned cubes in a given leaf order
(cube_enumerator), so that the definition can be exercised without a device.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from .ray_ref import Source, as_source, read_source     # noqa: F401 (re-exported)

OK, SKIPPED, BAD_WORLD, BAD_BOX = 0, -1, -2, -3
NONE = (0xFFFFFFFF, 0xFFFFFFFF)


def box_ref(enumerate_world: Callable, num_worlds: int, bundles: int, boxes_per_bundle: int,
            max_hits: int, *, lo, hi, centre: Source, world: Optional[Source] = None,
            bundles_per_world: int = 0, count: Optional[Source] = None):
    """(status int32 [B], count int32 [B], hits uint32 [B, K, 2]) of the query
    described in the module docstring."""
    F, G, K = int(bundles), int(boxes_per_bundle), int(max_hits)
    if F < 1 or G < 1 or K < 1:
        raise ValueError(f"{F} bundles of {G} boxes with {K} hits each")
    if F * G * K > 0x7FFFFFFF:
        raise ValueError(f"{F} x {G} x {K} is more than {0x7FFFFFFF} handles")
    if count is not None and bundles_per_world <= 0:
        raise ValueError("a count source needs bundles_per_world > 0")
    if bundles_per_world <= 0 and world is None:
        raise ValueError("no world source and no bundles_per_world")
    B = F * G
    lo = np.ascontiguousarray(lo, dtype=np.float32).reshape(B, 3)
    hi = np.ascontiguousarray(hi, dtype=np.float32).reshape(B, 3)
    status = np.zeros(B, np.int32)
    counts = np.zeros(B, np.int32)
    hits = np.full((B, K, 2), 0xFFFFFFFF, np.uint32)
    for f in range(F):
        boxes = slice(f * G, (f + 1) * G)
        if bundles_per_world > 0:
            w = f // bundles_per_world
        else:
            w = int(read_source(world, f, np.int32, 1)[0])
        if not 0 <= w < num_worlds:
            status[boxes] = BAD_WORLD
            continue
        if count is not None and \
                f % bundles_per_world >= int(read_source(count, w, np.int32, 1)[0]):
            status[boxes] = SKIPPED
            continue
        c = read_source(centre, f, np.float32, 3)
        if not np.isfinite(c).all():
            status[boxes] = BAD_BOX
            continue
        for b in range(f * G, (f + 1) * G):
            with np.errstate(over="ignore", invalid="ignore"):
                p_min = (c + lo[b]).astype(np.float32)
                p_max = (c + hi[b]).astype(np.float32)
            if not (np.isfinite(lo[b]).all() and np.isfinite(hi[b]).all() and
                    np.isfinite(p_min).all() and np.isfinite(p_max).all() and
                    (p_min <= p_max).all()):
                status[b] = BAD_BOX
                continue
            found = enumerate_world(w, p_min, p_max)
            if found is None:
                continue
            counts[b] = len(found)
            for k, entity in enumerate(found[:K]):
                hits[b, k] = np.asarray(entity, np.int64).astype(np.uint32)     # (gen, id)
    return status, counts, hits


def cube_enumerator(worlds: Sequence[Optional[Sequence[Tuple[Sequence[float], Sequence[float],
                                                             Tuple[int, int]]]]]):
    """enumerate_world() over axis-aligned boxes: worlds[w] is a list of (p_min,
    p_max, (gen, id)) in the tree's traversal order, or None for a tree that
    was never built.  Strict comparisons, as AABB::overlaps and the hull test:
    boxes that only touch do not overlap."""
    def enumerate_world(w, q_min, q_max):
        if worlds[w] is None:
            return None
        out = []
        for p_min, p_max, entity in worlds[w]:
            p_min = np.asarray(p_min, np.float32)
            p_max = np.asarray(p_max, np.float32)
            if (q_min < p_max).all() and (p_min < q_max).all():
                out.append(tuple(entity))
        return out
    return enumerate_world
