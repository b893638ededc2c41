"""CPU-only: <madrona/navmesh.hpp> and the utils.hpp pieces it rests on.

* API conformance: a device TU and a host TU name every member
  (tests/shims/navmesh_conformance*), and the struct layout is the reference's.
* The host compile of the overlay (libnavmesh_host_test.so) against the
  fixture recorded from the reference's navmesh.cpp (tests/golden/
  navmesh_ref.npz, see README_navmesh.md) and against the numpy restatement
  (tests/navmesh_restate.py), bit for bit: triangles, adjacency (an edge of
  four triangles included), alias table, sampled points and polygons, BFS
  orders, Dijkstra distances, entry points and pop orders.
* Degenerate inputs: zero-area triangles are never sampled; polygons of the
  other island stay at FLT_MAX.
"""
import ctypes as C
import os

import numpy as np
import pytest

import navmesh_restate as R
import navmesh_shims as S
from madrona_amd.simlib import HIP_BUILD_DIR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "navmesh_ref.npz")


@pytest.fixture(scope="module")
def host(built):
    return S.host_lib()


@pytest.fixture(scope="module")
def rng(built):
    return R.Rand()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _case(gold, ci):
    return {k.split("/", 1)[1]: gold[k] for k in gold.files if k.startswith(f"c{ci}/")}


def test_conformance_layout(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libnavmesh_conformance.so"))
    out = np.zeros(16, np.uint64)
    lib.navconf_layout(C.c_void_p(out.ctypes.data))
    # reference include/madrona/navmesh.hpp: four pointers, two counts; the
    # search states' pointers in declaration order
    assert out.tolist() == [40, 0, 8, 16, 24, 32, 36, 8, 4, 24, 16, 8, 32, 8, 24,
                            0xFFFFFFFF]
    lib.navconf_square.restype = C.c_uint32
    assert lib.navconf_square() == 202


def test_host_build_matches_reference(host, gold):
    for ci in range(len(gold["cases"])):
        g = _case(gold, ci)
        r = S.host_run(host, g["verts"], g["idxs"], g["offsets"], g["sizes"],
                       g["keys"], float(gold["radius2"]))
        for k in ("tri_idx", "adjacency", "tau", "alias"):
            assert np.array_equal(S.bits(r[k]), S.bits(g[k])), (ci, k)
        assert np.array_equal(S.bits(r["verts_out"]), S.bits(g["verts"])), ci
        T = len(g["tau"])
        S.assert_queries_equal(r, g, [T] * len(g["keys"]), ("host", ci))


def test_restatement_matches_reference(rng, gold):
    for ci in range(len(gold["cases"])):
        g = _case(gold, ci)
        m = R.build(g["verts"], g["idxs"], g["offsets"], g["sizes"])
        for k, mine in (("tri_idx", m.tri_idx), ("adjacency", m.adjacency),
                        ("tau", m.tau), ("alias", m.alias)):
            assert np.array_equal(S.bits(mine), S.bits(g[k])), (ci, k)
        r = S.restate_run(rng, [m], np.zeros(len(g["keys"]), int), g["keys"],
                          gold["radius2"])
        S.assert_queries_equal(r, g, [m.num_tris] * len(g["keys"]), ("restate", ci))


def test_fixture_covers_the_edge_cases(gold):
    fams = gold["cases"][:, 0]
    # the fin family: one edge of four triangles -- the first triangle's side of
    # it names the last one, the second and third still name the first
    g = _case(gold, int(np.nonzero(fams == 3)[0][0]))
    adj, tri = g["adjacency"], g["tri_idx"]
    edges = {}
    for t in range(len(tri)):
        for e in range(3):
            a, b = int(tri[t, e]), int(tri[t, (e + 1) % 3])
            edges.setdefault((min(a, b), max(a, b)), []).append((t, e))
    shared = [v for v in edges.values() if len(v) == 4]
    assert len(shared) == 1
    (t0, e0), (t1, e1), (t2, e2), (t3, e3) = shared[0]
    assert adj[t0, e0] == t3 and adj[t1, e1] == t0 and adj[t2, e2] == t0 \
        and adj[t3, e3] == t0
    # the grid family: exactly tied path lengths, a single triangle: BFS over
    # a queue of capacity one sees it empty at once (as in the reference)
    g = _case(gold, int(np.nonzero(fams == 4)[0][0]))
    assert (g["bfs_count"] == 0).all() and (g["pop_count"] == 1).all()


def test_host_matches_restatement_many_keys(host, rng, built):
    from madrona_amd.simlib import hip_lib_path
    sim = C.CDLL(hip_lib_path("navmesh_agents"), mode=C.RTLD_LOCAL)
    for fam in range(5):
        for world in (2, 5):
            _, v, i, o, s = R.agents_polygons(sim, world, 17, fam + 1)
            keys = np.array([rng.split((fam, world), q) for q in range(96)], np.uint32)
            r = S.host_run(host, v, i, o, s, keys, R.BFS_RADIUS2)
            m = R.build(v, i, o, s)
            for k, mine in (("tri_idx", m.tri_idx), ("adjacency", m.adjacency),
                            ("tau", m.tau), ("alias", m.alias)):
                assert np.array_equal(S.bits(r[k]), S.bits(mine)), (fam, k)
            want = S.restate_run(rng, [m], np.zeros(len(keys), int), keys, R.BFS_RADIUS2)
            S.assert_queries_equal(r, want, [m.num_tris] * len(keys), (fam, world))


def test_degenerate_inputs(host, rng):
    # zero-area fan triangles (a vertex in the middle of an edge) and a mesh
    # of two islands
    verts = np.array([[0, 0, 0], [0.5, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0],
                      [5, 0, 0], [6, 0, 0], [6, 1, 0]], np.float32)
    idxs = np.array([0, 1, 2, 3, 4, 2, 1, 0, 5, 6, 7], np.uint32)
    offsets = np.array([0, 5, 8], np.uint32)
    sizes = np.array([5, 3, 3], np.uint32)
    keys = np.array([rng.split((1, 2), q) for q in range(2000)], np.uint32)
    r = S.host_run(host, verts, idxs, offsets, sizes, keys, 100.0)
    m = R.build(verts, idxs, offsets, sizes)
    A = verts[m.tri_idx[:, 0]]
    area2 = np.linalg.norm(np.cross(verts[m.tri_idx[:, 1]] - A, verts[m.tri_idx[:, 2]] - A),
                           axis=1)
    zero = np.nonzero(area2 == 0)[0]
    assert len(zero) >= 2
    assert not np.isin(r["polys"], zero).any()
    island = m.num_tris - 1
    from_main = r["polys"] != island
    assert (r["distances"][from_main][:, island] == np.finfo(np.float32).max).all()
    assert (r["distances"][~from_main][:, :island] == np.finfo(np.float32).max).all()
    assert from_main.any() and (~from_main).any()
