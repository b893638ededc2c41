"""ctypes bindings of the navmesh test shims (tests/shims/navmesh_*) and the
comparison helpers the CPU and GPU navmesh tests share."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import navmesh_restate as R
from madrona_amd.simlib import HIP_BUILD_DIR

P, U = C.c_void_p, C.c_uint32


def host_lib():
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libnavmesh_host_test.so"))
    lib.nav_host_build.restype = P
    lib.nav_host_build.argtypes = [P, U, P, P, P, U]
    lib.nav_host_num_tris.restype = U
    lib.nav_host_num_tris.argtypes = [P]
    lib.nav_host_read.argtypes = [P] * 6
    lib.nav_host_sample.argtypes = [P, P, U, P, P]
    lib.nav_host_bfs.argtypes = [P, P, P, C.c_float, U, P, P]
    lib.nav_host_dijkstra.argtypes = [P, P, P, U, P, P, P, P, P]
    lib.nav_host_free.argtypes = [P]
    return lib


def c(a):
    return np.ascontiguousarray(a).ctypes.data


def host_run(lib, verts, idxs, offsets, sizes, keys, radius2):
    """Builds on the host and runs sampling, BFS and Dijkstra for keys."""
    verts = np.ascontiguousarray(verts, np.float32)
    idxs = np.ascontiguousarray(idxs, np.uint32)
    offsets = np.ascontiguousarray(offsets, np.uint32)
    sizes = np.ascontiguousarray(sizes, np.uint32)
    keys = np.ascontiguousarray(keys, np.uint32)
    h = lib.nav_host_build(c(verts), len(verts), c(idxs), c(offsets), c(sizes),
                           len(sizes))
    try:
        T = lib.nav_host_num_tris(h)
        Q = len(keys)
        r = dict(tri_idx=np.zeros((T, 3), np.uint32), adjacency=np.zeros((T, 3), np.uint32),
                 tau=np.zeros(T, np.float32), alias=np.zeros(T, np.uint32),
                 verts_out=np.zeros_like(verts), points=np.zeros((Q, 3), np.float32),
                 polys=np.zeros(Q, np.uint32), bfs_order=np.zeros((Q, T), np.uint32),
                 bfs_count=np.zeros(Q, np.uint32), distances=np.zeros((Q, T), np.float32),
                 entries=np.zeros((Q, T, 3), np.float32), pop_order=np.zeros((Q, T), np.uint32),
                 pop_dist=np.zeros((Q, T), np.float32), pop_count=np.zeros(Q, np.uint32))
        lib.nav_host_read(h, c(r["tri_idx"]), c(r["adjacency"]), c(r["tau"]),
                          c(r["alias"]), c(r["verts_out"]))
        lib.nav_host_sample(h, c(keys), Q, c(r["points"]), c(r["polys"]))
        lib.nav_host_bfs(h, c(r["polys"]), c(r["points"]), C.c_float(radius2), Q,
                         c(r["bfs_order"]), c(r["bfs_count"]))
        lib.nav_host_dijkstra(h, c(r["polys"]), c(r["points"]), Q, c(r["distances"]),
                              c(r["entries"]), c(r["pop_order"]), c(r["pop_dist"]),
                              c(r["pop_count"]))
        return r
    finally:
        lib.nav_host_free(h)


def restate_run(rng, meshes, mesh_of_query, keys, radius2):
    """The same through the numpy restatement, queries over several meshes."""
    pack = R.Pack(meshes)
    mesh_of_query = np.asarray(mesh_of_query, np.int64)
    pts, polys = R.sample(rng, pack, mesh_of_query, keys)
    bo, bc = R.bfs(pack, mesh_of_query, polys, pts, radius2)
    d, e, po, pd, pc = R.dijkstra(pack, mesh_of_query, polys, pts)
    return dict(points=pts, polys=polys, bfs_order=bo, bfs_count=bc, distances=d,
                entries=e, pop_order=po, pop_dist=pd, pop_count=pc, pack=pack)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32)


def assert_queries_equal(got, want, T_of_query, label):
    """got / want: dicts of per-query arrays (rows padded to different widths);
    compared bit for bit over each query's triangles."""
    assert np.array_equal(bits(got["points"]), bits(want["points"])), (label, "points")
    assert np.array_equal(bits(got["polys"]), bits(want["polys"])), (label, "polys")
    assert np.array_equal(bits(got["bfs_count"]), bits(want["bfs_count"])), (label, "bfs count")
    assert np.array_equal(bits(got["pop_count"]), bits(want["pop_count"])), (label, "pops")
    for q, T in enumerate(T_of_query):
        nb, npop = int(want["bfs_count"][q]), int(want["pop_count"][q])
        assert np.array_equal(bits(got["bfs_order"][q, :nb]),
                              bits(want["bfs_order"][q, :nb])), (label, q, "bfs order")
        assert np.array_equal(bits(got["pop_order"][q, :npop]),
                              bits(want["pop_order"][q, :npop])), (label, q, "pop order")
        assert np.array_equal(bits(got["pop_dist"][q, :npop]),
                              bits(want["pop_dist"][q, :npop])), (label, q, "pop dist")
        assert np.array_equal(bits(got["distances"][q, :T]),
                              bits(want["distances"][q, :T])), (label, q, "distances")
        assert np.array_equal(bits(got["entries"][q, :T]),
                              bits(want["entries"][q, :T])), (label, q, "entries")
