"""Shared by tests/test_mesh_bvh_cpu.py and tests/test_mesh_bvh_gpu.py: ctypes
bindings of the mesh_cast manager's probes (sims/mesh_cast/mgr.cpp; the
reference's MeshBVH code in oracle/_ref/libmesh_cast_ref.so, the header
overlay's host path in libmesh_cast_hip.so), the trees they return, and the
seeded query batches."""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from madrona_amd.simlib import HIP_BUILD_DIR, hip_lib_path, ref_lib_path

P, U = C.c_void_p, C.c_uint32

NUM_WORLD_FAMILIES = 5      # single triangle, box room, floor, height field, ellipsoid
NUM_FAMILIES = 7            # + two triangles, 4097 triangles
TRIS_PER_LEAF = 2
NODE_BYTES = 60
FLT_MAX = np.float32(np.finfo(np.float32).max)

NUM_RAYS, NUM_SWEEPS, NUM_BOXES = 4096, 1024, 256
PROBE_HEIGHT = np.float32(10.0)

NODE_DTYPE = np.dtype([
    ("minPoint", np.float32, 3), ("exp", np.int8, 3), ("numChildren", np.uint8),
    ("triSize", np.uint8, 4),
    ("qMinX", np.uint8, 4), ("qMinY", np.uint8, 4), ("qMinZ", np.uint8, 4),
    ("qMaxX", np.uint8, 4), ("qMaxY", np.uint8, 4), ("qMaxZ", np.uint8, 4),
    ("children", np.uint32, 4)])
assert NODE_DTYPE.itemsize == NODE_BYTES


def c(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _bind(path):
    lib = C.CDLL(path)
    lib.mesh_cast_num_families.restype = U
    lib.mesh_cast_tree_info.restype = C.c_int32
    lib.mesh_cast_tree_info.argtypes = [U, P, P]
    lib.mesh_cast_tree_arrays.argtypes = [U, P, P, P]
    lib.mesh_cast_source_tris.argtypes = [U, P, P, P]
    lib.mesh_cast_trace.argtypes = [U, U] + [P] * 9
    lib.mesh_cast_sweep.argtypes = [U, U] + [P] * 6
    lib.mesh_cast_overlap.argtypes = [U, U] + [P] * 4
    lib.mesh_cast_construct.argtypes = [U] + [P] * 5
    return lib


@functools.lru_cache(maxsize=None)
def ref_lib():
    path = ref_lib_path("mesh_cast")
    assert os.path.exists(path), f"{path}: the reference build of sims/mesh_cast is missing"
    return _bind(path)


@functools.lru_cache(maxsize=None)
def hip_host_lib():
    return _bind(hip_lib_path("mesh_cast"))


class Tree:
    """A family's built tree, read out of a probe library."""

    def __init__(self, lib, family):
        counts = np.zeros(5, np.uint32)
        root = np.zeros(6, np.float32)
        self.material_idx = lib.mesh_cast_tree_info(family, c(counts), c(root))
        (self.num_nodes, self.num_leaves, self.num_verts, self.num_padded_verts,
         self.num_src_tris) = (int(v) for v in counts)
        self.root = root
        self.nodes_raw = np.zeros(self.num_nodes * NODE_BYTES, np.uint8)
        self.materials = np.zeros(self.num_verts // 3, np.int32)
        self.vertices = np.zeros((self.num_padded_verts, 5), np.float32)
        lib.mesh_cast_tree_arrays(family, c(self.nodes_raw), c(self.materials),
                                  c(self.vertices))
        self.nodes = self.nodes_raw.view(NODE_DTYPE)
        self.src_pos = np.zeros((self.num_src_tris, 3, 3), np.float32)
        self.src_uv = np.zeros((self.num_src_tris, 3, 2), np.float32)
        self.src_mat = np.zeros(self.num_src_tris, np.int32)
        lib.mesh_cast_source_tris(family, c(self.src_pos), c(self.src_uv),
                                  c(self.src_mat))


@functools.lru_cache(maxsize=None)
def ref_tree(family):
    return Tree(ref_lib(), family)


# ---------------------------------------------------------------------------
# query batches

def _dirs(rng, n):
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[:, 2] = -np.abs(d[:, 2])      # mostly downwards: the meshes face up / out
    return d


@functools.lru_cache(maxsize=None)
def ray_batch(family):
    """4096 rays: aimed at the mesh's box from around and above it; free ones;
    rays with zero direction components; rays starting inside the scene's box
    and exactly on its faces / on the floor plane; rays with a t_max shorter
    than the scene; and one ray straight down onto every point of the integer
    grid [-7, 7]^2 (over the height field: exactly through an interior
    vertex)."""
    rng = np.random.default_rng(1000 + family)
    tree = ref_tree(family)
    n = NUM_RAYS
    o = np.empty((n, 3), np.float32)
    o[:, :2] = rng.uniform(-5, 5, (n, 2))
    o[:, 2] = rng.uniform(1.5, 6, n)
    d = _dirs(rng, n)
    t_max = np.full(n, FLT_MAX, np.float32)

    k = np.arange(n)
    aimed = k % 8 < 3
    lo, hi = tree.root[:3], tree.root[3:]
    target = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d[aimed] = (target - o)[aimed]

    zero = k % 8 == 3
    o[zero, :2] = rng.uniform(-3, 3, (int(zero.sum()), 2))
    mask = rng.integers(1, 7, n)    # bit a set: component a stays
    for a in range(3):
        d[zero & ((mask >> a) & 1 == 0), a] = 0.0

    inside = k % 8 == 4
    o[inside] = rng.uniform([-4, -4, 0], [4, 4, 4], (int(inside.sum()), 3))
    d[inside] = rng.normal(size=(int(inside.sum()), 3))
    face = inside & (k % 16 == 4)
    axis = rng.integers(0, 3, n)
    side = rng.integers(0, 2, n)
    for a in range(3):
        sel = face & (axis == a)
        o[sel, a] = np.where(side[sel] == 1, 4.0, 0.0 if a == 2 else -4.0)

    short = k % 8 == 5
    t_max[short] = rng.uniform(0.05, 1.0, int(short.sum()))

    g = np.arange(-7, 8, dtype=np.float32)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    num_grid = gx.size
    o[n - num_grid:, 0] = gx.ravel()
    o[n - num_grid:, 1] = gy.ravel()
    o[n - num_grid:, 2] = PROBE_HEIGHT
    d[n - num_grid:] = (0.0, 0.0, -1.0)
    t_max[n - num_grid:] = FLT_MAX

    assert (np.abs(d).max(axis=1) > 0).all()
    return (np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32),
            t_max, n - num_grid)


@functools.lru_cache(maxsize=None)
def sweep_batch(family):
    """1024 sweeps, radii 0.05 and 0.5 alternating: towards the mesh's box;
    free ones; ones with zero components; ones that start within the radius of
    a point of a mesh triangle (t = 0); t_max 1 or, for one in eight,
    FLT_MAX."""
    rng = np.random.default_rng(2000 + family)
    tree = ref_tree(family)
    n = NUM_SWEEPS
    k = np.arange(n)
    r = np.where(k % 2 == 0, 0.05, 0.5).astype(np.float32)
    o = np.empty((n, 3), np.float32)
    o[:, :2] = rng.uniform(-3.8, 3.8, (n, 2))
    o[:, 2] = rng.uniform(0.6, 3.5, n)
    d = (_dirs(rng, n) * rng.uniform(0.2, 2.0, (n, 1))).astype(np.float32)
    t_max = np.where(k % 8 == 7, FLT_MAX, np.float32(1.0)).astype(np.float32)

    aimed = (k // 2) % 4 == 0
    target = rng.uniform(tree.root[:3], tree.root[3:], (n, 3)).astype(np.float32)
    d[aimed] = ((target - o) * rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32))[aimed]

    zero = (k // 2) % 4 == 1
    mask = rng.integers(1, 7, n)
    for a in range(3):
        d[zero & ((mask >> a) & 1 == 0), a] = 0.0

    touch = (k // 2) % 4 == 2
    tri = tree.src_pos[rng.integers(0, tree.num_src_tris, n)]
    w = rng.dirichlet((1.0, 1.0, 1.0), n).astype(np.float32)
    on_mesh = (tri * w[:, :, None]).sum(axis=1)
    offset = rng.normal(size=(n, 3))
    offset *= (rng.uniform(0.0, 0.9, n) * r / np.linalg.norm(offset, axis=1))[:, None]
    o[touch] = (on_mesh + offset)[touch]

    assert (np.abs(d).max(axis=1) > 0).all()
    return (np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32),
            r, t_max, touch)


@functools.lru_cache(maxsize=None)
def box_batch(family):
    rng = np.random.default_rng(3000 + family)
    n = NUM_BOXES
    centre = rng.uniform([-5, -5, -0.5], [5, 5, 4.5], (n, 3))
    half = rng.uniform(0.1, 2.0, (n, 3))
    half[::8] = 20.0        # the whole mesh
    return np.ascontiguousarray(np.concatenate([centre - half, centre + half], axis=1),
                                np.float32)


# ---------------------------------------------------------------------------
# running the batches through a probe library (the first `count` of each)

def run_rays(lib, family, count=None):
    o, d, t_max, _ = ray_batch(family)
    n = len(o) if count is None else count
    out = dict(hit=np.zeros(n, np.uint32), t=np.zeros(n, np.float32),
               normal=np.zeros((n, 3), np.float32), uv=np.zeros((n, 2), np.float32),
               leaf_mat=np.zeros(n, np.uint32), material=np.zeros(n, np.uint32))
    lib.mesh_cast_trace(family, n, c(o), c(d), c(t_max), c(out["hit"]), c(out["t"]),
                        c(out["normal"]), c(out["uv"]), c(out["leaf_mat"]),
                        c(out["material"]))
    return out


def run_sweeps(lib, family, count=None):
    o, d, r, t_max, _ = sweep_batch(family)
    n = len(o) if count is None else count
    out = dict(t=np.zeros(n, np.float32), normal=np.zeros((n, 3), np.float32))
    lib.mesh_cast_sweep(family, n, c(o), c(d), c(r), c(t_max), c(out["t"]),
                        c(out["normal"]))
    return out


def run_boxes(lib, family, count=None):
    boxes = box_batch(family)
    n = len(boxes) if count is None else count
    out = dict(count=np.zeros(n, np.uint32), sum=np.zeros((n, 3), np.float32),
               hash=np.zeros(n, np.uint32))
    lib.mesh_cast_overlap(family, n, c(boxes), c(out["count"]), c(out["sum"]),
                          c(out["hash"]))
    return out


@functools.lru_cache(maxsize=None)
def ref_results(family):
    """The reference's answers to the three batches; computed once."""
    lib = ref_lib()
    res = dict(rays=run_rays(lib, family), sweeps=run_sweeps(lib, family),
               boxes=run_boxes(lib, family))
    for group in res.values():
        for a in group.values():
            a.setflags(write=False)
    return res


def assert_same(got, want, label, count=None):
    """Bit for bit, field by field, over the first `count` queries."""
    for name, w in want.items():
        g = got[name]
        w = w if count is None else w[:count]
        gb, wb = bits(g).reshape(len(g), -1), bits(w).reshape(len(w), -1)
        bad = np.nonzero((gb != wb).any(axis=1))[0]
        assert len(bad) == 0, (label, name, f"{len(bad)} of {len(w)} differ", bad[:8],
                               g[bad[:4]], w[bad[:4]])


def device_shim_path():
    return os.path.join(HIP_BUILD_DIR, "libmesh_bvh_device_test.so")
