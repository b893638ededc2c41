"""GPU: the batch ray caster (madrona_amd/csrc/render_raycast.hip) on the edge
scenes of sims/raycast_probe against the float64 definition of its image
(tests/raycast_f64.py) -- no oracle library, no reference tree: the HIP
libraries, the golden records (tests/golden/raycast_probe_records.npz, which
test_raycast_probe_cpu.py pins to the reference CPU backend and analyses) and
numpy.

On the pixels float64 calls decided -- all five rays of the pixel agree on every
discrete outcome -- hit masks are equal without exception, depth agrees to
raycast_probe_utils.DEPTH_RTOL and colour to one 8-bit step; the undecided ones
are left out and counted against the caps the CPU test holds the scenes to.
A failure names the scene kind (world w builds kind w % 16)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import raycast_f64 as F
import raycast_probe_utils as U
from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib

pytestmark = pytest.mark.gpu

DEPTH_ONLY, ASSET_FORM, TOO_DEEP = 1 << 1, 1 << 3, 1 << 5


def _kinds(worlds):
    return [w % U.KINDS for w in range(worlds) for _ in range(2)]


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(U.GOLDEN) as gold:
        return {k: gold[k] for k in gold.files}


_geometry = {}


@functools.lru_cache(maxsize=None)
def _want(res):
    """float64 images of the golden records: once per resolution"""
    gold = _golden()
    return F.render_worlds(_geometry["geo"], gold["instances"], gold["inst_counts"],
                           gold["views"], gold["lights"], gold["light_counts"], res)


def _assert_golden_rows(records, worlds=U.KINDS):
    """The scene analysed on the CPU is the scene in the HIP tables: per world the
    same instance rows and codes as multisets, the same views and lights in
    order, bit for bit."""
    gold = _golden()
    n_inst, n_light = int(gold["inst_counts"].sum()), int(gold["light_counts"].sum())
    assert np.array_equal(records["inst_counts"][:U.KINDS], gold["inst_counts"])
    assert np.array_equal(records["light_counts"][:U.KINDS], gold["light_counts"])
    for key, got in (("instances", records["instances"][:n_inst]),
                     ("views", records["views"][:2 * U.KINDS]),
                     ("lights", records["lights"][:n_light]),
                     ("codes", records["codes"][:n_inst])):
        assert np.array_equal(got, gold[key]), key
    assert worlds % U.KINDS == 0
    assert np.array_equal(records["inst_counts"],
                          np.tile(gold["inst_counts"], worlds // U.KINDS))


def _render(sim, rgbd=True):
    """(depth only: the rgb column is four bytes a row, not an image)"""
    sim.render()
    return sim.read_tensor("depth").copy(), sim.read_tensor("rgb").copy() if rgbd else None


@functools.lru_cache(maxsize=None)
def _hip(res, flags=0):
    """16 worlds, one step, one render: depth, rgb (None: depth only), records"""
    with Simulator(hip_lib_path("raycast_probe"), U.KINDS, flags=flags | (res << 8)) as sim:
        _geometry.setdefault("geo", U.sim_geometry(sim.lib))
        sim.step(1)
        depth, rgb = _render(sim, rgbd=not flags & DEPTH_ONLY)
        return depth, rgb, U.hip_records(sim)


def _log(case, stats):
    """$RAYCAST_PROBE_STATS_FILE collects, per scene kind, the undecided share,
    the largest relative depth error and the pixels one colour step off."""
    path = os.environ.get("RAYCAST_PROBE_STATS_FILE")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "kinds": {str(k): v for k, v in stats.items()}})
                    + "\n")


@pytest.mark.parametrize("res", [32, 33, 17, 8, 1])
def test_every_kind_against_float64(built, res):
    """res 32: whole tiles; 33: an odd size, a column and a row of one-pixel
    tiles, rays with a direction component of exactly 0; 17, 8, 1: partial
    tiles down to a single pixel."""
    depth, rgb, records = _hip(res)
    assert depth.shape == (2 * U.KINDS, res, res) and rgb.shape == (2 * U.KINDS, res, res, 4)
    _assert_golden_rows(records)
    _log(f"res{res}", U.compare_with_f64(depth, rgb, _want(res), _kinds(U.KINDS), res,
                                         ("res", res)))


def test_depth_only_gives_the_same_depth(built):
    depth, rgb, records = _hip(32, DEPTH_ONLY)
    _assert_golden_rows(records)
    assert rgb is None
    assert np.array_equal(depth.view(np.uint32), _hip(32)[0].view(np.uint32))
    U.compare_with_f64(depth, None, _want(32), _kinds(U.KINDS), 32, "depth only")


def test_asset_form_gives_the_same_bytes(built):
    depth, rgb, records = _hip(32, ASSET_FORM)
    _assert_golden_rows(records)
    assert np.array_equal(depth.view(np.uint32), _hip(32)[0].view(np.uint32))
    assert np.array_equal(rgb, _hip(32)[1])


def _tiles_per_workgroup(views, res, cus):
    """render_raycast.hip: buildRenderLaunches' grid and renderRaycast's runs"""
    per_view = ((res + 15) // 16) ** 2
    tiles = views * per_view
    grid = min(max(tiles, 1), min(max(views, 6 * cus), 65536))
    if views >= grid or views >= 2048:
        return -(-views // grid) * per_view, per_view
    return -(-tiles // grid), per_view


def test_workgroups_that_walk_from_world_to_world(built):
    """More than six tiles per CU: a workgroup takes a run of tiles that crosses
    views and worlds -- restaging LDS, between worlds it stages (<= 64
    instances) and the one it traces from HBM (kind 6), past worlds without
    instances or lights."""
    import torch
    res = 17
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    worlds = 512
    while _tiles_per_workgroup(2 * worlds, res, cus)[0] < 2:
        worlds *= 2
    run, per_view = _tiles_per_workgroup(2 * worlds, res, cus)
    assert worlds <= 4096 and run >= 2 and (run % per_view != 0 or run > per_view)
    with Simulator(hip_lib_path("raycast_probe"), worlds, flags=res << 8) as sim:
        _geometry.setdefault("geo", U.sim_geometry(sim.lib))
        rt = runtime_lib()
        rt.mwhip_device_cus.restype = C.c_uint32
        rt.mwhip_device_cus.argtypes = [C.c_void_p]
        assert rt.mwhip_device_cus(sim.hip_exec()) == cus
        sim.step(1)
        depth, rgb = _render(sim)
        _assert_golden_rows(U.hip_records(sim), worlds)
    first = 2 * U.KINDS
    _log("many worlds", U.compare_with_f64(depth[:first], rgb[:first], _want(res),
                                            _kinds(U.KINDS), res, "many worlds"))
    depth = depth.view(np.uint32).reshape(worlds // U.KINDS, first, res, res)
    rgb = rgb.reshape(worlds // U.KINDS, first, res, res, 4)
    same = (depth == depth[:1]).all((2, 3)) & (rgb == rgb[:1]).all((2, 3, 4))
    assert same.all(), ("views that differ from their kind's first (group, view)",
                        np.argwhere(~same)[:8].tolist())


def test_static_scene_renders_the_same_again(built):
    res = 32
    with Simulator(hip_lib_path("raycast_probe"), U.KINDS, flags=res << 8) as sim:
        sim.step(1)
        depth, rgb = _render(sim)
        again = _render(sim)
        sim.step(3)
        assert (sim.read_tensor("steps") == 4).all()
        later = _render(sim)
    for d, c in (again, later, _hip(res)[:2]):
        assert np.array_equal(d.view(np.uint32), depth.view(np.uint32))
        assert np.array_equal(c, rgb)


def test_a_tree_deeper_than_the_stack_is_an_error_or_right(built):
    """Kind 8 with 27 levels (flag bit 5; 86 instances, so primary rays walk the
    top-level tree): the walk needs more than the 24 stack entries a ray has.
    The overflow branches of traceWorld / traceInstance set kErrRender and drop
    the entry, nothing is written past the stack: either the replay reports it
    (mwhip_run returns non-zero, the message names the traversal stack) -- what
    the MI355X does: "device error 0x80: ray caster: ... a traversal stack
    overflowed" -- or no ray got that deep and every decided pixel is right.  A
    finished render with wrong pixels is the failure.  (mwhip_run directly:
    MWCudaExecutor::run treats an error as fatal, like the reference.)"""
    res = 32
    rt = runtime_lib()
    rt.mwhip_run.restype = C.c_int
    rt.mwhip_run.argtypes = [C.c_void_p, C.c_uint64]
    with Simulator(hip_lib_path("raycast_probe"), U.KINDS, flags=TOO_DEEP | (res << 8)) as sim:
        geo = U.sim_geometry(sim.lib)
        sim.step(1)
        records = U.hip_records(sim)
        assert records["inst_counts"][8] == U.TOO_DEEP_INSTANCES
        at = int(records["inst_counts"][:8].sum())
        codes = np.sort(records["codes"][at:at + U.TOO_DEEP_INSTANCES])
        assert U.worst_stack_need(U.karras_children(codes)) > U.STACK_DEPTH
        rc = rt.mwhip_run(sim.hip_exec(), sim.render_graph())
        if rc != 0:
            message = rt.mwhip_last_error().decode()
            assert "traversal stack" in message, (rc, message)
            print(f"too deep: mwhip_run -> {rc}: {message}")
            return
        depth, rgb = sim.read_tensor("depth"), sim.read_tensor("rgb")
    want = F.render_worlds(geo, records["instances"], records["inst_counts"], records["views"],
                           records["lights"], records["light_counts"], res, worlds=(8,))
    print("too deep: rendered without an error", U.compare_with_f64(
        depth[16:18], rgb[16:18], want, [8, 8], res, "too deep"))
