"""-m gpu: <madrona/navmesh.hpp> on the device (tests/shims/navmesh_device_shim.hip).

Meshes of every navmesh_agents family, built on the device by
Navmesh::initFromPolygons (one lane per mesh, persistent + scratch regions of
a stand-alone ecs_state) or on the host and copied over; then 4096 queries, one
lane each: samplePointAndPoly, bfsFromPoly and dijkstrasFromPoly.  Everything
is compared bit for bit with the numpy restatement (tests/navmesh_restate.py).
"""
import ctypes as C
import os

import numpy as np
import pytest

import navmesh_restate as R
import navmesh_shims as S
from madrona_amd.simlib import HIP_BUILD_DIR, hip_lib_path

pytestmark = pytest.mark.gpu

NUM_QUERIES = 4096


def _meshes(sim):
    polys = []
    for fam in range(5):
        for world in (0, 7, 40):
            polys.append(R.agents_polygons(sim, world, 9, fam + 1)[1:])
    return polys


@pytest.mark.parametrize("on_device", [1, 0], ids=["device_built", "host_built"])
def test_device_queries_match_restatement(built, on_device):
    from madrona_amd.simlib import _torch_runtime_first
    _torch_runtime_first()
    sim = C.CDLL(hip_lib_path("navmesh_agents"), mode=C.RTLD_LOCAL)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libnavmesh_device_test.so"))
    lib.nav_dev_run.restype = C.c_int32
    U, P = C.c_uint32, C.c_void_p
    lib.nav_dev_run.argtypes = [P, U, P, U, P, U, P, P, U, P, C.c_int32, P, P, U, U,
                                C.c_float] + [P] * 12

    polys = _meshes(sim)
    rows, verts, idxs, offs, sizes, tri_off = [], [], [], [], [], [0]
    nv = ni = npoly = 0
    meshes = []
    for v, i, o, s in polys:
        rows.append([nv, ni, npoly, len(v), len(s)])
        verts.append(v)
        idxs.append(i)
        offs.append(o)
        sizes.append(s)
        nv, ni, npoly = nv + len(v), ni + len(i), npoly + len(s)
        meshes.append(R.build(v, i, o, s))
        tri_off.append(tri_off[-1] + meshes[-1].num_tris)
    rows = np.array(rows, np.uint32)
    verts = np.concatenate(verts).astype(np.float32)
    idxs, offs, sizes = (np.concatenate(x).astype(np.uint32) for x in (idxs, offs, sizes))
    tri_off = np.array(tri_off, np.uint32)
    M, TT = len(meshes), int(tri_off[-1])
    tmax = max(m.num_tris for m in meshes)

    rng = R.Rand()
    qmesh = (np.arange(NUM_QUERIES) % M).astype(np.uint32)
    keys = np.array([rng.split((0xD0, on_device), q) for q in range(NUM_QUERIES)],
                    np.uint32)

    out = dict(tri_idx=np.zeros((TT, 3), np.uint32), adjacency=np.zeros((TT, 3), np.uint32),
               tau=np.zeros(TT, np.float32), alias=np.zeros(TT, np.uint32),
               verts=np.zeros_like(verts), query=np.zeros((NUM_QUERIES, 6), np.uint32),
               bfs_order=np.zeros((NUM_QUERIES, tmax), np.uint32),
               pop_order=np.zeros((NUM_QUERIES, tmax), np.uint32),
               pop_dist=np.zeros((NUM_QUERIES, tmax), np.float32),
               distances=np.zeros((NUM_QUERIES, tmax), np.float32),
               entries=np.zeros((NUM_QUERIES, tmax, 3), np.float32))
    used = np.zeros(2, np.uint64)
    c = S.c
    rc = lib.nav_dev_run(c(rows), M, c(verts), len(verts), c(idxs), len(idxs), c(offs),
                         c(sizes), len(sizes), c(tri_off), on_device, c(qmesh), c(keys),
                         NUM_QUERIES, tmax, R.BFS_RADIUS2, c(out["tri_idx"]),
                         c(out["adjacency"]), c(out["tau"]), c(out["alias"]),
                         c(out["verts"]), c(out["query"]), c(out["bfs_order"]),
                         c(out["pop_order"]), c(out["pop_dist"]), c(out["distances"]),
                         c(out["entries"]), c(used))
    assert rc == 0

    for m, mesh in enumerate(meshes):
        t0, t1 = int(tri_off[m]), int(tri_off[m + 1])
        for k, mine in (("tri_idx", mesh.tri_idx), ("adjacency", mesh.adjacency),
                        ("tau", mesh.tau), ("alias", mesh.alias)):
            assert np.array_equal(S.bits(out[k][t0:t1]), S.bits(mine)), (m, k)
    assert np.array_equal(out["verts"].view(np.uint32), verts.view(np.uint32))
    if on_device:
        # outputs only, one 128-B aligned block per mesh
        assert int(used[0]) == sum(R.device_block_bytes(len(p[0]), m.num_tris)
                                   for p, m in zip(polys, meshes))

    want = S.restate_run(rng, meshes, qmesh, keys, R.BFS_RADIUS2)
    q = out["query"]
    got = dict(points=q[:, :3].copy().view(np.float32), polys=q[:, 3],
               bfs_count=q[:, 4], pop_count=q[:, 5], bfs_order=out["bfs_order"],
               pop_order=out["pop_order"], pop_dist=out["pop_dist"],
               distances=out["distances"], entries=out["entries"])
    S.assert_queries_equal(got, want, [meshes[i].num_tris for i in qmesh],
                           ("device", on_device))
