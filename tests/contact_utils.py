"""Helpers of the contact-query tests (test_contact_ref_cpu.py,
test_contact_query_gpu.py): the reference's scalar narrowphase
(oracle/_ref/libphys_ref.so, ref_collide_pair) as the narrowphase that
madrona_amd/contact_ref.py takes, the objects of sims/contact_probe, worlds out
of a simulator's dump, and the brute force over all pairs."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from madrona_amd import contact_ref as cr
from madrona_amd.simlib import REF_BUILD_DIR

PHYS_REF = os.path.join(REF_BUILD_DIR, "libphys_ref.so")

# the unit-cube hull of sims/escape_room_phys and sims/contact_probe
CUBE_VERTS = np.array([
    [-.5, -.5, -.5], [.5, -.5, -.5], [.5, .5, -.5], [-.5, .5, -.5],
    [-.5, -.5, .5], [.5, -.5, .5], [.5, .5, .5], [-.5, .5, .5]], np.float32)
CUBE_IDX = np.array([0, 3, 2, 1, 4, 5, 6, 7, 0, 1, 5, 4,
                     2, 3, 7, 6, 0, 4, 7, 3, 1, 2, 6, 5], np.uint32)
CUBE_COUNTS = np.array([4] * 6, np.uint32)
SPHERE_RADIUS = 0.7     # the one sphere ref_collide_pair knows

STEPS = (1, 3, 12, 40)  # where the probe is compared
PROBE_WORLDS = 16
PROBE_SEED = 5
MAX_CONTACTS = 32       # the K of the GPU test


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def phys_ref():
    lib = C.CDLL(PHYS_REF)
    mesh = [C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
            C.c_uint32]
    lib.ref_bake_objects.restype = C.c_int32
    lib.ref_bake_objects.argtypes = mesh + [
        C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32,
        C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]
    lib.ref_collide_pair.restype = None
    lib.ref_collide_pair.argtypes = mesh + [C.POINTER(C.c_float), C.POINTER(C.c_float),
                                            C.c_int32, C.POINTER(C.c_float)]
    return lib


def probe_objects(lib):
    """contact_probe's objects (Cube, Plane, Sphere) as contact_ref takes them,
    the primitives' boxes as the reference's asset baker makes them"""
    types = np.array([0, 1, 2], np.int32)       # the baker's: hull, plane, sphere
    inv_mass = np.array([1, 0, 1], np.float32)
    radius = np.array([0, 0, SPHERE_RADIUS], np.float32)
    floats = np.zeros(1024, np.float32)
    hedges = np.zeros(1024, np.uint32)
    n = lib.ref_bake_objects(
        _ptr(CUBE_VERTS, C.c_float), len(CUBE_VERTS), _ptr(CUBE_IDX, C.c_uint32),
        _ptr(CUBE_COUNTS, C.c_uint32), len(CUBE_COUNTS), _ptr(types, C.c_int32),
        _ptr(inv_mass, C.c_float), _ptr(radius, C.c_float), 3, _ptr(floats, C.c_float),
        len(floats), _ptr(hedges, C.c_uint32), len(hedges))
    assert n > 0
    boxes = floats[3 * 13: 3 * 13 + 3 * 6].reshape(3, 6).copy()
    kinds = (cr.HULL, cr.PLANE, cr.SPHERE)
    return [[{"type": kinds[o], "aabb": boxes[o]}] for o in range(3)]


def _txfm(side):
    return np.concatenate([side["position"], side["rotation"], side["scale"]]).astype(np.float32)


def ref_narrowphase(lib, calls=None):
    """ref_collide_pair as contact_ref's narrowphase (cube hulls, the plane, the
    sphere of radius 0.7); calls: a list that receives every pair sent"""
    def narrowphase(a, b):
        kinds = (a["prim"]["type"], b["prim"]["type"])
        mode = {(cr.HULL, cr.HULL): 0, (cr.HULL, cr.PLANE): 1, (cr.SPHERE, cr.HULL): 2}.get(kinds)
        if mode is None:
            raise cr.Unsupported(kinds)
        out = np.zeros(28, np.float32)
        ta, tb = _txfm(a), _txfm(b)
        lib.ref_collide_pair(
            _ptr(CUBE_VERTS, C.c_float), len(CUBE_VERTS), _ptr(CUBE_IDX, C.c_uint32),
            _ptr(CUBE_COUNTS, C.c_uint32), len(CUBE_COUNTS), _ptr(ta, C.c_float),
            _ptr(tb, C.c_float), mode, _ptr(out, C.c_float))
        if calls is not None:
            calls.append((kinds, out.copy()))
        if out[0] == 0:
            return None
        return bool(out[1]), int(out[2]), out[3:6].copy(), out[6:22].reshape(4, 4).copy()
    return narrowphase


def worlds_of_dump(dump, table: str = "Body"):
    """A list of contact_ref worlds out of Simulator.dump_all() of a simulator
    whose table `table` dumps what contact_probe's does"""
    def column(name, dtype, width):
        rows, counts = dump[f"{table}.{name}"]
        return rows.view(dtype).reshape(len(rows), width), counts

    entity, counts = column("Entity", np.int32, 2)
    position, _ = column("Position", np.float32, 3)
    rotation, _ = column("Rotation", np.float32, 4)
    scale, _ = column("Scale", np.float32, 3)
    object_id, _ = column("ObjectID", np.int32, 1)
    response, _ = column("ResponseType", np.int32, 1)
    presolve = None
    if f"{table}.PreSolvePositional" in dump:
        presolve, _ = column("PreSolvePositional", np.float32, 7)
    worlds, first = [], 0
    for n in counts:
        rows = slice(first, first + int(n))
        world = {"entity": entity[rows], "position": position[rows], "rotation": rotation[rows],
                 "scale": scale[rows], "object_id": object_id[rows, 0],
                 "response": response[rows, 0]}
        if presolve is not None:
            world["presolve"] = presolve[rows]
        worlds.append(world)
        first += int(n)
    return worlds


def _bounding_radius(world, k, objects):
    """float64, conservative: of every primitive of body k about its position;
    inf for a plane"""
    scale = np.abs(np.asarray(world["scale"][k], np.float64))
    radius = 0.0
    for prim in objects[int(world["object_id"][k])]:
        if prim["type"] == cr.PLANE:
            return np.inf
        box = np.asarray(prim["aabb"], np.float64)
        corner = np.maximum(np.abs(box[:3]), np.abs(box[3:])) * scale
        radius = max(radius, float(np.linalg.norm(corner)))
    return radius * (1 + 1e-5) + 1e-4


def brute_force(world, objects, narrowphase, poses="current"):
    """Every body pair that is not Static-Static and whose bounding spheres
    meet, every primitive pair of it, straight to the narrowphase: NO box test.
    Same tuples, same order as contact_ref.world_contacts."""
    n = len(world["object_id"])
    entity = np.asarray(world["entity"]).reshape(n, 2)
    poses_of = [cr.body_pose(world, k, poses) for k in range(n)]
    radii = [_bounding_radius(world, k, objects) for k in range(n)]
    out = []
    for k_lo in range(n):
        for k_hi in range(k_lo + 1, n):
            if world["response"][k_lo] == cr.STATIC and world["response"][k_hi] == cr.STATIC:
                continue
            apart = np.linalg.norm(poses_of[k_lo][0].astype(np.float64) -
                                   poses_of[k_hi][0].astype(np.float64))
            if apart > radii[k_lo] + radii[k_hi]:
                continue
            k_a, k_b = (k_lo, k_hi) if entity[k_lo, 1] < entity[k_hi, 1] else (k_hi, k_lo)
            for a_prim in objects[int(world["object_id"][k_a])]:
                for b_prim in objects[int(world["object_id"][k_b])]:
                    sides = []
                    for k, prim in ((k_a, a_prim), (k_b, b_prim)):
                        sides.append({"body": k, "position": poses_of[k][0],
                                      "rotation": poses_of[k][1],
                                      "scale": np.asarray(world["scale"][k], np.float32),
                                      "prim": prim})
                    a, b = sides
                    if a["prim"]["type"] > b["prim"]["type"]:
                        a, b = b, a
                    found = narrowphase(a, b)
                    if found is None or found[1] < 1:
                        continue
                    ref_is_a, num_points, normal, points = found
                    if a["prim"]["type"] != cr.HULL or b["prim"]["type"] != cr.HULL:
                        ref_is_a = False
                    ref, alt = (a, b) if ref_is_a else (b, a)
                    pts = np.zeros((4, 4), np.float32)
                    pts[:num_points] = np.asarray(points, np.float32).reshape(4, 4)[:num_points]
                    out.append((entity[ref["body"]].copy(), entity[alt["body"]].copy(),
                                int(num_points), np.asarray(normal, np.float32).copy(), pts))
    return out


def same_contacts(a, b) -> bool:
    """two lists of contact tuples, bit for bit"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if not (np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] and
                np.array_equal(x[3].view(np.uint32), y[3].view(np.uint32)) and
                np.array_equal(x[4].view(np.uint32), y[4].view(np.uint32))):
            return False
    return True
