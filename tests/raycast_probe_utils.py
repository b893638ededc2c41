"""Shared by the ray-caster probe tests (sims/raycast_probe): the records of the
reference CPU backend in a canonical form, the simulator's geometry, a Karras
radix tree over Morton codes, and the comparison of an image with
raycast_f64.  Test infrastructure only."""
import ctypes as C
import os

import numpy as np

from raycast_utils import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raycast_probe_records.npz")

KINDS = 16
# scene kind -> instances, lights (sims/raycast_probe/sim.cpp)
INSTANCE_COUNTS = [0, 1, 2, 5, 63, 64, 65, 17, 66, 5, 4, 5, 2, 2, 4, 30]
LIGHT_COUNTS = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 8, 9, 3, 1]
TOO_DEEP_INSTANCES = 86
# kind 8: pairs of codes down a chain, and fillers next to the root
DEEP_FILLERS = 32
# meaningful bytes of a record: the rest is alignment padding
INSTANCE_BYTES = 56
VIEW_BYTES = 44
LIGHT_BYTES = [b for b in range(40) if b not in (2, 3, 37, 38, 39)]
# the traversal stack of the ray caster, both levels (render_raycast.hip kStackDepth)
STACK_DEPTH = 24

# Tolerances of the GPU tests, set by what the stand-in oracle (the reference's
# own fp32 ray caster compiled for the host) shows against float64 on decided
# pixels of these scenes; tests/test_raycast_probe_cpu.py measures and asserts
# both figures.  Its largest relative depth error is 1.403e-5 -- not below 5e-6,
# where the project's 1e-5 would hold -- and fp32 cannot be held tighter than the
# reference's own fp32 code achieves: depth is held to twice that.  It has no
# pixel more than one 8-bit step off: colour is held to one step, none beyond.
ORACLE_DEPTH_ERROR = 1.403e-5
DEPTH_RTOL = 2 * ORACLE_DEPTH_ERROR
COLOUR_STEPS = 1


def sim_geometry(lib):
    """The meshes / materials a simulator's manager hands to the ray caster."""
    f = lib.sim_render_geometry
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p] * 7
    counts = np.zeros(3, np.uint32)
    n_obj = f(None, None, None, None, None, None, counts.ctypes.data)
    verts = np.zeros((counts[0], 3), np.float32)
    idx = np.zeros((counts[1], 3), np.uint32)
    voff = np.zeros(n_obj + 1, np.uint32)
    toff = np.zeros(n_obj + 1, np.uint32)
    mats = np.zeros((counts[2], 3), np.float32)
    omat = np.zeros(n_obj, np.int32)
    f(verts.ctypes.data, idx.ctypes.data, voff.ctypes.data, toff.ctypes.data,
      mats.ctypes.data, omat.ctypes.data, None)
    g = lib.sim_render_geometry_ex
    g.restype = C.c_int32
    g.argtypes = [C.c_void_p] * 6
    tcounts = np.zeros(2, np.uint32)
    n_tex = g(None, None, None, None, None, tcounts.ctypes.data)
    uvs = np.zeros((counts[0], 2), np.float32)
    tri_mats = np.zeros(counts[1], np.int32)
    mat_tex = np.zeros(max(counts[2], 1), np.int32)
    dims = np.zeros((max(n_tex, 1), 2), np.uint32)
    texels = np.zeros(max(int(tcounts[1]), 4), np.uint8)
    g(uvs.ctypes.data, tri_mats.ctypes.data, mat_tex.ctypes.data, dims.ctypes.data,
      texels.ctypes.data, None)
    textures, at = [], 0
    for t in range(n_tex):
        w, h = int(dims[t, 0]), int(dims[t, 1])
        textures.append((w, h, texels[at:at + 4 * w * h].copy()))
        at += 4 * w * h
    return Geometry(verts, idx, voff, toff, omat, mats, vertex_uvs=uvs,
                    triangle_materials=tri_mats, material_textures=mat_tex[:counts[2]],
                    textures=textures)


def sorted_rows(rows):
    """rows [n, bytes] in lexicographic order: a multiset in a canonical form"""
    if len(rows) == 0:
        return rows
    return rows[np.lexsort(rows.T[::-1])]


def canonical(instances, inst_counts, views, lights, light_counts, codes):
    """Records grouped by world in a form that does not depend on the order in
    which a backend keeps a world's instances, with the padding zeroed."""
    instances = np.ascontiguousarray(instances).reshape(-1, 64).copy()
    instances[:, INSTANCE_BYTES:] = 0
    views = np.ascontiguousarray(views).reshape(-1, 48).copy()
    views[:, VIEW_BYTES:] = 0
    lights = np.ascontiguousarray(lights).reshape(-1, 40).copy()
    keep = np.zeros(40, bool)
    keep[LIGHT_BYTES] = True
    lights[:, ~keep] = 0
    codes = np.ascontiguousarray(codes).view(np.uint32).ravel().copy()
    at = np.concatenate([[0], np.cumsum(inst_counts)])
    for w in range(len(inst_counts)):
        instances[at[w]:at[w + 1]] = sorted_rows(instances[at[w]:at[w + 1]])
        codes[at[w]:at[w + 1]] = np.sort(codes[at[w]:at[w + 1]])
    return {"instances": instances, "inst_counts": np.asarray(inst_counts, np.int32),
            "views": views, "lights": lights,
            "light_counts": np.asarray(light_counts, np.int32), "codes": codes}


def ref_records(worlds=KINDS, flags=0):
    """The reference CPU backend's records after one step, canonical, and the
    simulator's geometry."""
    from madrona_amd.simlib import Simulator, ref_lib_path
    with Simulator(ref_lib_path("raycast_probe"), worlds, num_workers=1, flags=flags) as ref:
        ref.step(1)
        f = ref.lib.render_prep_bridge_records
        f.restype = C.c_int64
        f.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64]
        got = []
        for kind, size in ((0, 64), (1, 48)):
            cap = worlds * 128
            rec = np.zeros((cap, size), np.uint8)
            keys = np.zeros(cap, np.uint64)
            n = f(kind, rec.ctypes.data, keys.ctypes.data, cap)
            assert n >= 0
            order = np.argsort(keys[:n], kind="stable")     # by world, then entity id
            # (an entity is appended by instanceTransformUpdate with the render
            # entity's default material, then once more by ...WithMat with its
            # overrides: the later record is the one a renderer ends up with)
            sorted_keys = keys[:n][order]
            last = np.append(sorted_keys[1:] != sorted_keys[:-1], True) if n else order
            order = order[last]
            world = (keys[:n][order] >> np.uint64(32)).astype(np.int64)
            got.append((rec[:n][order], np.bincount(world, minlength=worlds)))
        d = ref.dump_all()
        lights, light_counts = d["Light.LightDesc"]
        codes, code_counts = d["Renderable.MortonCode"]
        assert np.array_equal(code_counts, got[0][1])
        assert (got[1][1] == 2).all()
        geo = sim_geometry(ref.lib)
    return canonical(got[0][0], got[0][1], got[1][0], lights, light_counts, codes), geo


def hip_records(sim):
    """The HIP backend's tables in the same form."""
    d = sim.dump_all()
    inst, inst_counts = d["Renderable.InstanceData"]
    views, view_counts = d["Camera.PerspectiveCameraData"]
    lights, light_counts = d["Light.LightDesc"]
    codes, code_counts = d["Renderable.MortonCode"]
    assert np.array_equal(code_counts, inst_counts) and (view_counts == 2).all()
    return canonical(inst, inst_counts, views, lights, light_counts, codes)


# ---- Karras radix tree over sorted codes (what renderTlasBuild builds) -----------
def _lcp(codes, i, j):
    n = len(codes)
    if j < 0 or j >= n:
        return -1
    a, b = int(codes[i]), int(codes[j])
    if a != b:
        return 32 - (a ^ b).bit_length()
    return 32 + 32 - (i ^ j).bit_length()


def karras_children(codes):
    """children[i] = (left, right) of internal node i; a leaf k is -(k + 1)"""
    n = len(codes)
    children = []
    for i in range(n - 1):
        d = 1 if _lcp(codes, i, i + 1) - _lcp(codes, i, i - 1) >= 0 else -1
        delta_min = _lcp(codes, i, i - d)
        l_max = 2
        while _lcp(codes, i, i + l_max * d) > delta_min:
            l_max *= 2
        l, t = 0, l_max // 2
        while t >= 1:
            if _lcp(codes, i, i + (l + t) * d) > delta_min:
                l += t
            t //= 2
        j = i + l * d
        delta_node = _lcp(codes, i, j)
        s, t = 0, (l + 1) // 2
        while True:
            if _lcp(codes, i, i + (s + t) * d) > delta_node:
                s += t
            if t == 1:
                break
            t = (t + 1) // 2
        gamma = i + s * d + min(d, 0)
        lo, hi = min(i, j), max(i, j)
        children.append((-(gamma + 1) if lo == gamma else gamma,
                         -(gamma + 2) if hi == gamma + 1 else gamma + 1))
    return children


def worst_stack_need(children, node=0):
    """Most nodes with two internal children on a root-to-leaf path: what a
    near-first walk that defers the far child may have on its stack."""
    if not children:
        return 0
    left, right = children[node]
    below = max([worst_stack_need(children, c) for c in (left, right) if c >= 0] or [0])
    return below + (1 if left >= 0 and right >= 0 else 0)


def median_split_stack_need(triangles, leaf=4):
    """The same for the bottom-level tree of an object: median splits down to
    leaves of at most `leaf` triangles (render_raycast.hip buildBlas)."""
    if triangles <= leaf:
        return 0
    half = triangles // 2
    parts = (half, triangles - half)
    both = all(p > leaf for p in parts)
    return max(median_split_stack_need(p, leaf) for p in parts) + (1 if both else 0)


# ---- an image against the definition ----------------------------------------------
def undecided_caps(res):
    """undecided pixels allowed per view and per scene kind (two views): none at
    one pixel, two per view at res 8, 3 % of a kind's pixels above"""
    if res == 1:
        return 0, 0
    if res == 8:
        return 2, 4
    return 2 * res * res, int(0.03 * 2 * res * res)


def compare_with_f64(depth, rgb, want, kinds_of_views, res, what):
    """depth [V,res,res] f32 and rgb [V,res,res,4] u8 (None: depth only) against
    raycast_f64.render_worlds' result for the same views.  Returns per scene kind
    (undecided share, largest relative depth error, pixels one step off)."""
    w_depth, w_rgb, decided = want[:3]
    assert depth.shape == w_depth.shape
    stats = {}
    for kind in sorted(set(kinds_of_views)):
        v = np.flatnonzero(np.asarray(kinds_of_views) == kind)
        ok = decided[v]
        undecided = int((~ok).sum())
        per_view, per_kind = undecided_caps(res)
        assert len(v) == 2 and undecided <= per_kind and \
            ((~ok).sum((1, 2)) <= per_view).all(), (what, "kind", kind, "undecided", undecided)
        hit, w_hit = depth[v] > 0, w_depth[v] > 0
        flips = int((hit != w_hit)[ok].sum())
        assert flips == 0, (what, "kind", kind, "hit / miss flips on decided pixels", flips,
                            np.argwhere((hit != w_hit) & ok)[:8].tolist())
        both = ok & w_hit
        rel = np.abs(depth[v][both] - w_depth[v][both]) / w_depth[v][both]
        worst = float(rel.max()) if rel.size else 0.0
        assert worst <= DEPTH_RTOL, (what, "kind", kind, "depth", worst)
        assert (depth[v][~hit] == 0).all()
        one_off = 0
        if rgb is not None:
            assert (rgb[v][..., 3] == 255).all(), (what, "kind", kind, "alpha")
            assert (rgb[v][~hit][:, :3] == 0).all(), (what, "kind", kind, "a miss is black")
            diff = np.abs(rgb[v][..., :3].astype(np.int32) -
                          w_rgb[v][..., :3].astype(np.int32)).max(-1)
            beyond = int((diff[ok] > COLOUR_STEPS).sum())
            assert beyond == 0, (what, "kind", kind, "colour", beyond, int(diff[ok].max()),
                                 np.argwhere((diff > COLOUR_STEPS) & ok)[:8].tolist())
            one_off = int((diff[ok] == 1).sum())
        stats[kind] = (undecided / ok.size, worst, one_off)
    return stats
