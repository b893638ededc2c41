"""CPU-only: MeshBVH queries, builder and node quantisation of the header overlay
(<madrona/mesh_bvh.hpp>, mesh_bvh_builder.hpp) on the host.

* Builder invariants on the five mesh families of sims/mesh_cast plus a
  2-triangle and a 4097-triangle mesh; the reference-CPU build of the simulator
  gets the same tree bytes.
* The overlay's host queries against the reference's own (the mesh_cast
  manager's probes, see tests/mesh_bvh_utils.py), bit for bit: 4096 rays, 1024
  sweeps, 256 boxes per family.
* Conditions on the reference's output itself, so the batches exercise what
  they claim to: hit / miss shares, contacts at t = 0, the height field's
  vertex rays.
* QBVHNode::construct / convertToAABB against the reference's.
* API conformance: a device TU and a host TU name every added member
  (tests/shims/mesh_bvh_conformance*).
"""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_bvh_utils as M
from madrona_amd.simlib import HIP_BUILD_DIR

FAMILIES = list(range(M.NUM_FAMILIES))
WORLD_FAMILIES = list(range(M.NUM_WORLD_FAMILIES))
MAX_DEPTH = 11


@pytest.fixture(scope="module")
def libs(built):
    return M.ref_lib(), M.hip_host_lib()


def _scale(exp):
    return np.ldexp(np.float32(1.0), int(exp)).astype(np.float32)


def _child_box(node, i):
    """QBVHNode::convertToAABB in fp32: minPoint + 2^exp * q, two roundings."""
    lo, hi = np.empty(3, np.float32), np.empty(3, np.float32)
    for a, (qmin, qmax) in enumerate((("qMinX", "qMaxX"), ("qMinY", "qMaxY"),
                                      ("qMinZ", "qMaxZ"))):
        s = _scale(node["exp"][a])
        lo[a] = node["minPoint"][a] + np.float32(s * np.float32(node[qmin][i]))
        hi[a] = node["minPoint"][a] + np.float32(s * np.float32(node[qmax][i]))
    return lo, hi


def _walk(tree, node_idx, depth, seen_nodes, leaves):
    """Checks node node_idx and everything beneath; returns the positions
    beneath it and the deepest level of internal nodes reached."""
    assert node_idx < tree.num_nodes
    assert node_idx not in seen_nodes
    seen_nodes.add(node_idx)
    node = tree.nodes[node_idx]
    assert np.isfinite(node["minPoint"]).all()
    assert (node["exp"] >= -126).all()      # (int8: <= 127 anyway)
    n = int(node["numChildren"])
    assert 1 <= n <= 4
    beneath, deepest = [], depth
    for i in range(4):
        child = int(node["children"][i])
        if i >= n:
            assert child == 0xFFFFFFFF
            assert node["triSize"][i] == 0
            continue
        assert child != 0xFFFFFFFF
        if child & 0x80000000:
            first, size = child & 0x7FFFFFFF, int(node["triSize"][i])
            assert 1 <= size <= M.TRIS_PER_LEAF
            assert 3 * (first + size) <= tree.num_verts
            leaves.append((first, size))
            pos = tree.vertices[3 * first:3 * (first + size), :3]
        else:
            assert node["triSize"][i] == 0
            pos, d = _walk(tree, child, depth + 1, seen_nodes, leaves)
            deepest = max(deepest, d)
        lo, hi = _child_box(node, i)
        assert np.isfinite(lo).all() and np.isfinite(hi).all()
        assert (lo <= pos).all() and (pos <= hi).all(), (node_idx, i, lo, hi)
        beneath.append(pos)
    return np.concatenate(beneath), deepest


def _rows(pos, uv, mat):
    """Triangles as sortable byte rows (positions, uvs, material)."""
    n = len(mat)
    rows = np.concatenate([M.bits(pos).reshape(n, 9), M.bits(uv).reshape(n, 6),
                           mat.view(np.uint32).reshape(n, 1)], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


@pytest.mark.parametrize("family", FAMILIES)
def test_builder_invariants(libs, family):
    tree = M.Tree(libs[1], family)
    expected_tris = {0: 1, 1: 12, 2: 2, 3: 512, 5: 2, 6: 4097}
    if family in expected_tris:
        assert tree.num_src_tris == expected_tris[family]

    seen, leaves = set(), []
    pos, deepest = _walk(tree, 0, 1, seen, leaves)
    print(f"family {family}: {tree.num_src_tris} triangles, {tree.num_nodes} nodes, "
          f"{tree.num_leaves} leaves, depth {deepest}")

    # 3: counts; the leaves tile the triangle array in order, none twice
    assert len(seen) == tree.num_nodes
    assert len(leaves) == tree.num_leaves
    assert tree.num_verts == 3 * tree.num_src_tris
    leaves.sort()
    firsts = np.array([f for f, _ in leaves])
    sizes = np.array([s for _, s in leaves])
    assert firsts[0] == 0
    assert np.array_equal(firsts[1:], (firsts + sizes)[:-1])
    assert firsts[-1] + sizes[-1] == tree.num_src_tris
    assert tree.material_idx == -1

    # 4: depth.  A median split over L leaves is ceil(log4(L)) levels deep (at
    # least one): nothing less is possible 4-wide, and a builder that went
    # deeper would show here long before it reached the bound.
    assert deepest <= MAX_DEPTH
    want_depth = 1
    while 4 ** want_depth < tree.num_leaves:
        want_depth += 1
    assert tree.num_leaves == -(-tree.num_src_tris // M.TRIS_PER_LEAF)
    assert deepest == want_depth
    assert deepest == {0: 1, 1: 2, 2: 1, 3: 4, 4: 4, 5: 1, 6: 6}[family]

    # 2: the root box is the mesh's exact bounds
    src = tree.src_pos.reshape(-1, 3)
    assert np.array_equal(tree.root[:3], src.min(axis=0))
    assert np.array_equal(tree.root[3:], src.max(axis=0))
    assert len(pos) == tree.num_verts

    # what is in the leaves is the mesh: positions, uvs, materials
    nt = tree.num_src_tris
    got = _rows(tree.vertices[:3 * nt, :3].reshape(nt, 3, 3),
                tree.vertices[:3 * nt, 3:].reshape(nt, 3, 2), tree.materials)
    assert np.array_equal(got, _rows(tree.src_pos, tree.src_uv, tree.src_mat))

    # 6: the padded tail
    assert tree.num_padded_verts == tree.num_verts + 3 * (M.TRIS_PER_LEAF - 1)
    tail = tree.vertices[tree.num_verts:].reshape(-1, 3, 5)
    assert len(tail) == M.TRIS_PER_LEAF - 1
    assert (M.bits(tail) == M.bits(tree.vertices[tree.num_verts - 3:tree.num_verts])).all()

    # 7 / 5
    if family == 0:
        assert tree.num_nodes == 1 and tree.num_leaves == 1
        assert tree.nodes[0]["numChildren"] == 1
    if family == 2:
        assert tree.root[2] == tree.root[5] == 0.0
        assert tree.nodes[0]["exp"][2] == -126
        assert (tree.nodes[0]["qMinZ"] == 0).all() and (tree.nodes[0]["qMaxZ"] == 0).all()
    if family == 4:
        assert len(set(tree.src_mat.tolist())) == 5
        assert (tree.src_uv != 0).all()


@pytest.mark.parametrize("family", FAMILIES)
def test_same_tree_in_the_reference_build(libs, family):
    ref, hip = M.Tree(libs[0], family), M.Tree(libs[1], family)
    assert np.array_equal(ref.nodes_raw, hip.nodes_raw)
    assert np.array_equal(M.bits(ref.vertices), M.bits(hip.vertices))
    assert np.array_equal(ref.materials, hip.materials)
    assert np.array_equal(M.bits(ref.root), M.bits(hip.root))
    assert (ref.num_nodes, ref.num_leaves, ref.num_verts) == \
        (hip.num_nodes, hip.num_leaves, hip.num_verts)


@pytest.mark.parametrize("family", WORLD_FAMILIES)
def test_host_queries_match_reference(libs, family):
    want = M.ref_results(family)
    hip = libs[1]
    M.assert_same(M.run_rays(hip, family), want["rays"], ("rays", family))
    M.assert_same(M.run_sweeps(hip, family), want["sweeps"], ("sweeps", family))
    M.assert_same(M.run_boxes(hip, family), want["boxes"], ("boxes", family))


@pytest.mark.parametrize("family", WORLD_FAMILIES)
def test_reference_output_covers_the_cases(libs, family):
    """Conditions on the reference's answers: the batches hit, miss, touch."""
    res = M.ref_results(family)
    rays, sweeps, boxes = res["rays"], res["sweeps"], res["boxes"]
    o, d, t_max, grid_start = M.ray_batch(family)

    hit_share = rays["hit"].mean()
    print(f"family {family}: rays hit {hit_share:.3f}")
    assert hit_share >= 0.20
    if family != 1:
        assert 1.0 - hit_share >= 0.10
    assert not np.isnan(rays["t"]).any() and not np.isnan(rays["normal"]).any()
    assert (rays["t"][rays["hit"] == 1] <= t_max[rays["hit"] == 1]).all()

    so, sd, sr, st_max, touch = M.sweep_batch(family)
    contact_share = (sweeps["t"] < st_max).mean()
    print(f"family {family}: sweeps in contact before t_max {contact_share:.3f}, "
          f"at t = 0 {(sweeps['t'] == 0).mean():.3f}")
    assert contact_share >= 0.10
    assert not np.isnan(sweeps["t"]).any() and not np.isnan(sweeps["normal"]).any()
    # sweeps that start within the radius of the mesh touch at t = 0
    assert (sweeps["t"][touch] == 0).all()
    assert touch.sum() >= M.NUM_SWEEPS // 8
    for r in (0.05, 0.5):
        assert ((sweeps["t"] < st_max) & (sr == np.float32(r))).sum() > 0

    tree = M.ref_tree(family)
    assert boxes["count"].max() == tree.num_src_tris        # the all-enclosing boxes
    assert (boxes["count"] == 0).any() or family == 1

    # a t_max shorter than the first hit: the ray misses, and hits beyond
    # t_max when given FLT_MAX
    n = len(o)
    full = dict(hit=np.zeros(n, np.uint32), t=np.zeros(n, np.float32),
                normal=np.zeros((n, 3), np.float32), uv=np.zeros((n, 2), np.float32),
                leaf_mat=np.zeros(n, np.uint32), material=np.zeros(n, np.uint32))
    libs[0].mesh_cast_trace(family, n, M.c(o), M.c(d),
                            M.c(np.full(n, M.FLT_MAX, np.float32)), M.c(full["hit"]),
                            M.c(full["t"]), M.c(full["normal"]), M.c(full["uv"]),
                            M.c(full["leaf_mat"]), M.c(full["material"]))
    cut = (rays["hit"] == 0) & (full["hit"] == 1)
    print(f"family {family}: rays cut short by t_max {int(cut.sum())}")
    assert cut.sum() > 0
    assert (full["t"][cut] > t_max[cut]).all()

    if family == 3:
        # straight down onto every interior grid vertex: hits exactly at its
        # height (on the field's border the reference's edge rule decides)
        height = np.full((17, 17), np.nan, np.float32)
        src = tree.src_pos.reshape(-1, 3)
        height[(src[:, 0] + 8).astype(int), (src[:, 1] + 8).astype(int)] = src[:, 2]
        sel = slice(grid_start, None)
        assert (rays["hit"][sel] == 1).all()
        want_t = (M.PROBE_HEIGHT - height[1:-1, 1:-1].ravel()).astype(np.float32)
        assert len(want_t) == len(rays["t"][sel]) == 225
        assert np.array_equal(M.bits(rays["t"][sel]), M.bits(want_t))


def test_construct_and_convert_match_reference(libs):
    rng = np.random.default_rng(77)
    n = 256
    num_children = rng.integers(1, 5, n).astype(np.uint32)
    centre = rng.uniform(-50, 50, (n, 4, 3))
    half = rng.uniform(0.01, 1.0, (n, 4, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 1, 1))
    boxes = np.ascontiguousarray(np.concatenate([centre - half, centre + half], axis=2),
                                 np.float32)
    idx = rng.integers(1, 1 << 20, (n, 4)).astype(np.int32)
    idx[rng.random((n, 4)) < 0.5] *= -1

    out = []
    for lib in libs:
        nodes = np.zeros(n * M.NODE_BYTES, np.uint8)
        deq = np.zeros((n, 4, 6), np.float32)
        lib.mesh_cast_construct(n, M.c(num_children), M.c(boxes), M.c(idx), M.c(nodes),
                                M.c(deq))
        out.append((nodes, deq))
    (ref_nodes, ref_deq), (hip_nodes, hip_deq) = out
    assert np.array_equal(ref_nodes, hip_nodes)
    assert np.array_equal(M.bits(ref_deq), M.bits(hip_deq))

    nodes = hip_nodes.view(M.NODE_DTYPE)
    for k in range(n):
        node = nodes[k]
        assert node["numChildren"] == num_children[k]
        for i in range(4):
            if i < num_children[k]:
                v = int(idx[k, i])
                want = (-v - 1) | 0x80000000 if v < 0 else v - 1
                assert node["children"][i] == want
            else:
                assert node["children"][i] == 0xFFFFFFFF
            lo, hi = _child_box(node, i)
            assert np.array_equal(M.bits(np.concatenate([lo, hi])), M.bits(hip_deq[k, i]))


def test_builder_rejects_what_it_cannot_quantise(built):
    """No triangle, a non-finite position, bounds whose extent overflows fp32:
    an empty MeshBVH, not a tree whose boxes do not hold."""
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmesh_bvh_conformance.so"))
    lib.meshbvhconf_build_nodes.restype = C.c_uint32
    lib.meshbvhconf_build_nodes.argtypes = [C.c_void_p, C.c_uint32]
    big = np.finfo(np.float32).max

    def nodes(tri):
        pos = np.ascontiguousarray(tri, np.float32)
        return lib.meshbvhconf_build_nodes(M.c(pos), len(pos) // 3)

    assert nodes([[0, 0, 0], [1, 0, 0], [0, 1, 0]]) == 1
    assert nodes(np.zeros((0, 3))) == 0
    assert nodes([[0, 0, 0], [np.inf, 0, 0], [0, 1, 0]]) == 0
    assert nodes([[0, 0, 0], [np.nan, 0, 0], [0, 1, 0]]) == 0
    assert nodes([[-big, 0, 0], [big, 0, 0], [0, 1, 0]]) == 0
    # the largest extent fp32 holds still quantises
    assert nodes([[0, 0, 0], [big, 0, 0], [0, big, 0]]) == 1


def test_construct_zero_extent_is_finite(libs):
    """The overlay's exponent clamp (the reference's formula is undefined here)."""
    boxes = np.zeros((1, 4, 6), np.float32)
    boxes[0, 0] = (-4, -4, 0, 4, 0, 0)
    boxes[0, 1] = (-4, 0, 0, 4, 4, 0)
    idx = np.array([[-1, -3, 0, 0]], np.int32)
    nodes = np.zeros(M.NODE_BYTES, np.uint8)
    deq = np.zeros((1, 4, 6), np.float32)
    libs[1].mesh_cast_construct(1, M.c(np.array([2], np.uint32)), M.c(boxes), M.c(idx),
                                M.c(nodes), M.c(deq))
    node = nodes.view(M.NODE_DTYPE)[0]
    assert node["exp"][2] == -126
    assert np.isfinite(deq).all()
    assert (deq[0, :2, 2] == 0).all() and (deq[0, :2, 5] == 0).all()
    assert (deq[0, :2, :3] <= boxes[0, :2, :3]).all()
    assert (deq[0, :2, 3:] >= boxes[0, :2, 3:]).all()


def test_conformance(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmesh_bvh_conformance.so"))
    out = np.zeros(24, np.uint64)
    lib.meshbvhconf_layout(C.c_void_p(out.ctypes.data))
    # reference include/madrona/mesh_bvh.hpp: QBVHNode, MeshBVH and its member
    # offsets, BVHVertex, LeafMaterial, RayIsectTxfm, HitInfo and its offsets,
    # TriangleIndices, numTrisPerLeaf, nodeWidth, sentinel
    assert out.tolist() == [60, 72, 0, 8, 16, 24, 48, 52, 56, 60, 64, 20, 4, 96,
                            40, 0, 4, 16, 24, 32, 12, 2, 4, 0xFFFFFFFF]
    lib.meshbvhconf_host_queries.restype = C.c_uint32
    assert lib.meshbvhconf_host_queries() == 1
