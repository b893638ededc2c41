"""Ray queries in numpy: the definition that mwhip_rays_* (include/mwhip.h,
csrc/ray_query.hip, include/madrona/phys_impl/ray_query.inl)
computes on the device, and the yardstick of its tests.  The tracer is
injected: this file defines everything AROUND a cast -- fans, sources and
strides, fans_per_world and counts, every status, the output conventions --
and `trace(world, o, d, t_max) -> (t, normal, entity) | None` says what a ray
meets (on the device: BVH::traceRay of world's broadphase tree; None for every
ray of a world whose tree no broadphase pass has built yet).

N = F * R rays, F fans of R >= 1 rays that share an origin and a world; ray
i = f * R + r is ray r of fan f.  A SOURCE is (buf, record_bytes, first_byte):
item k is read at byte k * record_bytes + first_byte of buf (uint8).

    world[f]    int32.  fans_per_world > 0 replaces it: world = f // fans_per_world.
    count[w]    optional int32 per world, only with fans_per_world > 0: fan f
                with f % fans_per_world >= count[world] is SKIPPED.
    origin[f]   3 float32.
    dir[i]      3 float32, used as given (hit_t is in units of its length).
    t_max[i]    float32.

Per ray, checked in this order and nothing behind a failed check is read:

    BAD_WORLD (-2)  world not in [0, num_worlds)
    SKIPPED   (-1)  by the count rule
    BAD_RAY   (-3)  a non-finite component of the origin; then, per ray, a
                    non-finite component of the direction, an all-zero
                    direction, a NaN t_max
    HIT (1) / MISS (0)  what trace() says

    hit_t[i]    float32, 0 on anything but a HIT
    hit[i]      uint32 [2] (gen, id), Entity::none() = (0xFFFFFFFF, 0xFFFFFFFF)
                on anything but a HIT
    normal[i]   3 float32, zero on anything but a HIT

Also here: a brute-force slab tracer over axis-aligned boxes (box_tracer), so
that the definition can be exercised without a device, and float32
restatements of Vector3::normalize and Quat::rotateVec (<madrona/math.hpp>,
compiled with -ffp-contract=off), from which the tests build the directions
the simulators' own ray systems use.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import numpy as np

HIT, MISS, SKIPPED, BAD_WORLD, BAD_RAY = 1, 0, -1, -2, -3
NONE = (0xFFFFFFFF, 0xFFFFFFFF)

Source = Tuple[np.ndarray, int, int]     # (uint8 buffer, record_bytes, first_byte)


def read_source(source: Source, k: int, dtype, items: int) -> np.ndarray:
    """Item k of a source: `items` values of `dtype` at k * record_bytes +
    first_byte."""
    buf, record_bytes, first_byte = source
    buf = np.ascontiguousarray(buf).view(np.uint8).ravel()
    nbytes = np.dtype(dtype).itemsize * items
    if record_bytes % 4 or first_byte % 4:
        raise ValueError("record_bytes and first_byte must be multiples of 4")
    if first_byte + nbytes > record_bytes:
        raise ValueError(f"{nbytes} bytes from byte {first_byte} do not fit a record of "
                         f"{record_bytes} bytes")
    at = k * record_bytes + first_byte
    return buf[at:at + nbytes].view(dtype).copy()


def as_source(array, dtype) -> Source:
    """A contiguous array of one item per row as a source."""
    array = np.ascontiguousarray(array, dtype=dtype)
    rows = array.shape[0]
    record = array.size * array.itemsize // max(rows, 1)
    return array.view(np.uint8).ravel(), record, 0


def ray_ref(trace: Callable, num_worlds: int, fans: int, rays_per_fan: int, *,
            directions, t_max, origin: Source, world: Optional[Source] = None,
            fans_per_world: int = 0, count: Optional[Source] = None):
    """(hit_t float32 [N], hit uint32 [N, 2], normal float32 [N, 3], status
    int32 [N]) of the query described in the module docstring."""
    F, R = int(fans), int(rays_per_fan)
    if F < 1 or R < 1:
        raise ValueError(f"{F} fans of {R} rays")
    if count is not None and fans_per_world <= 0:
        raise ValueError("a count source needs fans_per_world > 0")
    if fans_per_world <= 0 and world is None:
        raise ValueError("no world source and no fans_per_world")
    N = F * R
    directions = np.ascontiguousarray(directions, dtype=np.float32).reshape(N, 3)
    t_max = np.ascontiguousarray(t_max, dtype=np.float32).reshape(N)
    hit_t = np.zeros(N, np.float32)
    hit = np.full((N, 2), 0xFFFFFFFF, np.uint32)
    normal = np.zeros((N, 3), np.float32)
    status = np.zeros(N, np.int32)
    for f in range(F):
        rays = slice(f * R, (f + 1) * R)
        if fans_per_world > 0:
            w = f // fans_per_world
        else:
            w = int(read_source(world, f, np.int32, 1)[0])
        if not 0 <= w < num_worlds:
            status[rays] = BAD_WORLD
            continue
        if count is not None and f % fans_per_world >= int(read_source(count, w, np.int32, 1)[0]):
            status[rays] = SKIPPED
            continue
        o = read_source(origin, f, np.float32, 3)
        if not np.isfinite(o).all():
            status[rays] = BAD_RAY
            continue
        for i in range(f * R, (f + 1) * R):
            d = directions[i]
            if not np.isfinite(d).all() or not d.any() or np.isnan(t_max[i]):
                status[i] = BAD_RAY
                continue
            met = trace(w, o, d, t_max[i])
            if met is None:
                continue
            t, n, entity = met
            status[i] = HIT
            hit_t[i] = np.float32(t)
            normal[i] = np.asarray(n, np.float32)
            hit[i] = np.asarray(entity, np.int64).astype(np.uint32)     # (gen, id)
    return hit_t, hit, normal, status


def box_tracer(worlds: Sequence[Sequence[Tuple[Sequence[float], Sequence[float], Tuple[int, int]]]]):
    """trace() over axis-aligned boxes: worlds[w] is a list of (p_min, p_max,
    (gen, id)).  The closest entry point with 0 <= t <= t_max over the boxes
    whose OUTSIDE the origin is on (a ray that starts inside a box does not meet
    it, as a hull's back faces are not met); the normal is the face's.  float64
    slabs: a definition to read, not a pin of the device's rounding.  Ties go to
    the box listed first."""
    def trace(w, o, d, t_max):
        best = None
        o = np.asarray(o, np.float64)
        d = np.asarray(d, np.float64)
        for p_min, p_max, entity in worlds[w]:
            p_min = np.asarray(p_min, np.float64)
            p_max = np.asarray(p_max, np.float64)
            t_near, t_far, axis_near, sign = -np.inf, np.inf, -1, 0.0
            missed = False
            for a in range(3):
                if d[a] == 0.0:
                    if o[a] < p_min[a] or o[a] > p_max[a]:
                        missed = True
                        break
                    continue
                t0 = (p_min[a] - o[a]) / d[a]
                t1 = (p_max[a] - o[a]) / d[a]
                lo, hi = min(t0, t1), max(t0, t1)
                if lo > t_near:
                    t_near, axis_near, sign = lo, a, -1.0 if d[a] > 0 else 1.0
                t_far = min(t_far, hi)
            if missed or t_near > t_far or t_near < 0.0 or t_near > float(t_max):
                continue
            if best is None or t_near < best[0]:
                n = np.zeros(3, np.float32)
                n[axis_near] = sign
                best = (np.float32(t_near), n, entity)
        return best
    return trace


# ---- <madrona/math.hpp> in float32, operation by operation ------------------------
def _f32(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float32)


def normalize_f32(v) -> np.ndarray:
    """Vector3::normalize: v * (1.f / sqrtf(x * x + y * y + z * z)), [..., 3]."""
    v = _f32(v)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    length2 = (x * x + y * y) + z * z
    inv = np.float32(1) / np.sqrt(length2, dtype=np.float32)
    return np.stack([x * inv, y * inv, z * inv], -1).astype(np.float32)


def _cross_f32(a, b):
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    bx, by, bz = b[..., 0], b[..., 1], b[..., 2]
    return np.stack([ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx], -1)


def rotate_vec_f32(quat, v) -> np.ndarray:
    """Quat::rotateVec for quat = (w, x, y, z) [..., 4] and v [..., 3]:
    v + 2.f * (cross(pure, v) * w + cross(pure, cross(pure, v)))."""
    quat, v = _f32(quat), _f32(v)
    pure = quat[..., 1:4]
    scalar = quat[..., 0:1]
    pure_x_v = _cross_f32(pure, v)
    pure_x_pure_x_v = _cross_f32(pure, pure_x_v)
    return (v + np.float32(2) * ((pure_x_v * scalar) + pure_x_pure_x_v)).astype(np.float32)


def fan_direction_inputs(plan_mode: bool = False) -> np.ndarray:
    """What fanDirection (sims/broadphase_only/sim.cpp) normalizes, float32
    [32, 3]; in plan mode the first five rows are the axis-aligned directions
    it returns as they are."""
    i = np.arange(32)
    v = np.stack([((i * 7) % 11 - 5).astype(np.float32) + np.float32(0.5),
                  ((i * 3) % 13 - 6).astype(np.float32) + np.float32(0.25),
                  np.float32(0.75) * ((i % 5) - 2).astype(np.float32)], -1).astype(np.float32)
    if plan_mode:
        v[:5] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, -1]]
    return v


def fan_directions(plan_mode: bool = False) -> np.ndarray:
    """fanDirection(i, plan_mode) for i = 0 .. 31, float32 [32, 3]."""
    v = fan_direction_inputs(plan_mode)
    out = normalize_f32(v)
    if plan_mode:
        out[:5] = v[:5]
    return out
