"""-m gpu: MeshBVH's queries on the device against the reference's own.

* Device shim (tests/shims/mesh_bvh_device_shim.hip): the ray, sweep and box
  batches of tests/mesh_bvh_utils.py one query per lane over uploaded trees,
  every output field equal bit for bit to the reference's host probe
  (oracle/_ref/libmesh_cast_ref.so), for all five mesh families, at batch sizes
  1, 63, 64, 65 (partial wavefronts) and 4096.
* Lock step: the mesh_cast simulator on this backend against its build on the
  reference CPU backend, every dumped column after steps 1, 3 and 8, at 1, 2,
  65 and 1024 worlds (65 worlds: every family and every wrap of w % 5).
* Upload: the device block read back holds the host arrays and the padded
  tail, each array at a multiple of 128 bytes.
"""
import ctypes as C

import numpy as np
import pytest

import mesh_bvh_utils as M
from parity_utils import compare_columns
from madrona_amd.simlib import Simulator, hip_lib_path, ref_lib_path

pytestmark = pytest.mark.gpu

FAMILIES = list(range(M.NUM_WORLD_FAMILIES))
BATCHES = [1, 63, 64, 65, 4096]
P, U = C.c_void_p, C.c_uint32


@pytest.fixture(scope="module")
def dev(built):
    lib = C.CDLL(M.device_shim_path())
    lib.mbvh_dev_upload.restype = P
    lib.mbvh_dev_upload.argtypes = [C.c_int, P, U, P, P, U, U, P, C.c_int32]
    lib.mbvh_dev_free.argtypes = [P]
    lib.mbvh_dev_block.argtypes = [P, P, P, P]
    lib.mbvh_dev_trace.argtypes = [P, U] + [P] * 9
    lib.mbvh_dev_sweep.argtypes = [P, U] + [P] * 6
    lib.mbvh_dev_overlap.argtypes = [P, U] + [P] * 4
    return lib


@pytest.fixture(scope="module")
def uploaded(dev):
    """The reference build's trees, uploaded once."""
    handles = {}
    for f in FAMILIES:
        t = M.ref_tree(f)
        h = dev.mbvh_dev_upload(0, M.c(t.nodes_raw), t.num_nodes, M.c(t.materials),
                                M.c(t.vertices), t.num_verts, t.num_leaves, M.c(t.root),
                                t.material_idx)
        assert h, f"upload of family {f} failed"
        handles[f] = h
    yield handles
    for h in handles.values():
        dev.mbvh_dev_free(h)


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("family", FAMILIES)
def test_device_queries_match_reference(dev, uploaded, family, n):
    want = M.ref_results(family)
    h = uploaded[family]

    o, d, t_max, _ = M.ray_batch(family)
    n_rays = min(n, len(o))
    # the vertex rays sit at the batch's end: the small batches take them too
    sel = slice(len(o) - n_rays, len(o))
    o, d, t_max = (np.ascontiguousarray(a[sel]) for a in (o, d, t_max))
    got = dict(hit=np.zeros(n_rays, np.uint32), t=np.zeros(n_rays, np.float32),
               normal=np.zeros((n_rays, 3), np.float32), uv=np.zeros((n_rays, 2), np.float32),
               leaf_mat=np.zeros(n_rays, np.uint32), material=np.zeros(n_rays, np.uint32))
    assert dev.mbvh_dev_trace(h, n_rays, M.c(o), M.c(d), M.c(t_max), M.c(got["hit"]),
                              M.c(got["t"]), M.c(got["normal"]), M.c(got["uv"]),
                              M.c(got["leaf_mat"]), M.c(got["material"])) == 0
    M.assert_same(got, {k: v[sel] for k, v in want["rays"].items()}, ("rays", family, n))

    o, d, r, t_max, _ = M.sweep_batch(family)
    n_sw = min(n, len(o))
    got = dict(t=np.zeros(n_sw, np.float32), normal=np.zeros((n_sw, 3), np.float32))
    assert dev.mbvh_dev_sweep(h, n_sw, M.c(o), M.c(d), M.c(r), M.c(t_max), M.c(got["t"]),
                              M.c(got["normal"])) == 0
    M.assert_same(got, want["sweeps"], ("sweeps", family, n), count=n_sw)

    boxes = M.box_batch(family)
    n_bx = min(n, len(boxes))
    got = dict(count=np.zeros(n_bx, np.uint32), sum=np.zeros((n_bx, 3), np.float32),
               hash=np.zeros(n_bx, np.uint32))
    assert dev.mbvh_dev_overlap(h, n_bx, M.c(boxes), M.c(got["count"]), M.c(got["sum"]),
                                M.c(got["hash"])) == 0
    M.assert_same(got, want["boxes"], ("boxes", family, n), count=n_bx)


@pytest.mark.parametrize("family", FAMILIES)
def test_upload_block(dev, uploaded, family):
    t = M.ref_tree(family)
    offsets, sizes = np.zeros(3, np.uint64), np.zeros(2, np.uint64)
    assert dev.mbvh_dev_block(uploaded[family], M.c(offsets), M.c(sizes), None) == 0
    block = np.zeros(int(sizes[1]), np.uint8)
    assert dev.mbvh_dev_block(uploaded[family], M.c(offsets), M.c(sizes), M.c(block)) == 0

    assert offsets[0] == 0 and (offsets % 128 == 0).all()
    node_bytes = t.num_nodes * M.NODE_BYTES
    mat_bytes = 4 * (t.num_verts // 3)
    vert_bytes = 20 * t.num_padded_verts
    assert sizes[0] == vert_bytes
    assert offsets[1] >= node_bytes and offsets[2] >= offsets[1] + mat_bytes
    assert sizes[1] >= offsets[2] + vert_bytes

    o1, o2 = int(offsets[1]), int(offsets[2])
    assert np.array_equal(block[:node_bytes], t.nodes_raw)
    assert np.array_equal(block[o1:o1 + mat_bytes], t.materials.view(np.uint8))
    assert np.array_equal(block[o2:o2 + vert_bytes], t.vertices.view(np.uint8).ravel())
    # the padded tail: numTrisPerLeaf - 1 copies of the last triangle
    tail = block[o2 + 20 * t.num_verts:o2 + vert_bytes].view(np.float32).reshape(-1, 3, 5)
    last = t.vertices[t.num_verts - 3:t.num_verts]
    assert len(tail) == M.TRIS_PER_LEAF - 1
    assert (M.bits(tail) == M.bits(last)).all()
    # the gaps between the arrays are zero bytes
    assert not block[node_bytes:o1].any() and not block[o1 + mat_bytes:o2].any()


@pytest.mark.parametrize("num_worlds", [1, 2, 65, 1024])
def test_mesh_cast_lock_step(built, num_worlds):
    checkpoints = (1, 3, 8)
    with Simulator(ref_lib_path("mesh_cast"), num_worlds, seed=5, num_workers=1) as ref, \
            Simulator(hip_lib_path("mesh_cast"), num_worlds, seed=5) as hip:
        assert compare_columns(ref.dump_all(), hip.dump_all()) == []
        for step in range(1, max(checkpoints) + 1):
            ref.step(1)
            hip.step(1)
            if step in checkpoints:
                ref_dump, hip_dump = ref.dump_all(), hip.dump_all()
                assert compare_columns(ref_dump, hip_dump) == [], step
                if step == max(checkpoints) and num_worlds >= 65:
                    # the run exercised the queries: hits and misses, contacts
                    # and free moves, overlaps
                    rows = ref_dump["Agent.RayT"][0].view(np.uint32)
                    assert (rows == 0xFFFFFFFF).any() and (rows != 0xFFFFFFFF).any()
                    t = ref_dump["Agent.SweepResult"][0].view(np.float32).reshape(-1, 4)[:, 0]
                    assert (t < 1).any() and (t == 1).any()
                    cnt = ref_dump["Agent.OverlapResult"][0].view(np.uint32).reshape(-1, 4)[:, 0]
                    assert (cnt > 0).any()
        for name in ref.tensor_names:
            assert np.array_equal(ref.read_tensor(name).view(np.uint8),
                                  hip.read_tensor(name).view(np.uint8)), name
