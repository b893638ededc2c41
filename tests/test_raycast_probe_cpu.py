"""CPU: the scenes of sims/raycast_probe as the reference CPU backend records
them, and the two things the GPU test (test_raycast_probe_gpu.py) rests on.

1. The scenes ARE the edges they claim to be: instance and light counts, equal
   Morton codes, a Karras tree as deep as the traversal stack allows -- and few
   enough pixels are undecided (raycast_f64: the five rays of a pixel disagree
   about a discrete outcome) that leaving them out leaves the edges in.
2. The stand-in oracle (the reference's own ray caster compiled for the host,
   raycast_utils.ref_render) is pinned by the same float64 definition on the
   same records.  Measured here, 16 worlds at res 32 and res 33, decided pixels:
     hit / miss flips                          0
     largest relative depth error              1.403e-05 (res 32, kinds 4-6: the
                                               wall of small objects; at most
                                               6.9e-06 in every other kind)
     pixels more than one 8-bit step off       0 (one step off: 14)
   These set the GPU tolerances (raycast_probe_utils.DEPTH_RTOL, COLOUR_STEPS):
   the oracle's own depth error is not below 5e-6, so fp32 depth is held to
   twice its measured maximum, 2.806e-5; colour to one step, none beyond."""
import functools
import os

import numpy as np
import pytest

import raycast_f64 as F
import raycast_probe_utils as U
from madrona_amd.simlib import ref_lib_path
from raycast_utils import INSTANCE_DT, LIGHT_DT, REF_LIB, VIEW_DT, ref_render

pytestmark = pytest.mark.skipif(
    not (os.path.exists(ref_lib_path("raycast_probe")) and os.path.exists(REF_LIB)),
    reason="oracle/_ref not built")


@functools.lru_cache(maxsize=None)
def _records(flags=0):
    return U.ref_records(U.KINDS, flags)


@functools.lru_cache(maxsize=None)
def _f64(res, drop_light=None, worlds=None):
    rec, geo = _records()
    return F.render_worlds(geo, rec["instances"], rec["inst_counts"], rec["views"],
                           rec["lights"], rec["light_counts"], res, worlds=worlds,
                           drop_light=drop_light, decide=drop_light is None)


def _world_rows(rec, w, what="instances", counts="inst_counts"):
    at = np.concatenate([[0], np.cumsum(rec[counts])])
    return rec[what][at[w]:at[w + 1]]


def test_counts_and_shapes_of_every_kind():
    rec, geo = _records()
    assert rec["inst_counts"].tolist() == U.INSTANCE_COUNTS
    assert rec["light_counts"].tolist() == U.LIGHT_COUNTS
    inst = rec["instances"].view(INSTANCE_DT).ravel()
    # inside the geometry, no flat instance
    assert ((inst["objectID"] >= 0) & (inst["objectID"] < geo.num_objects)).all()
    assert (inst["scale"] > 0).all()
    # whatever is not a box is turned off every axis and scaled unevenly
    other = inst[inst["objectID"] != 0]
    assert set(other["objectID"].tolist()) == {1, 2, 3, 4}
    assert (np.abs(other["rotation"]) > 1e-3).all()
    assert (np.ptp(other["scale"], axis=1) > 0.05).all()
    # the fifth mesh has twelve triangles and is not its own bounding box
    tris = geo.triangle_offsets
    assert tris[5] - tris[4] == 12 and tris[1] - tris[0] == 12 and tris[2] - tris[1] == 168
    v = geo.vertices[geo.vertex_offsets[4]:geo.vertex_offsets[5]]
    assert len(np.unique(v[:, 0])) == 4
    # viewer 0: identity, 90 degrees; viewer 1: a general rotation, 60 degrees, offset
    views = rec["views"].view(VIEW_DT).ravel()
    assert views["worldIDX"].tolist() == [w for w in range(U.KINDS) for _ in range(2)]
    assert (views["rotation"][0::2] == [1, 0, 0, 0]).all()
    assert (np.abs(views["rotation"][1::2]) > 0.01).all()
    assert np.allclose(views["yScale"][0::2], -1.0, atol=1e-6)
    assert np.allclose(views["yScale"][1::2], -np.sqrt(3.0), atol=1e-6)
    assert (views["position"][1::2] == [1.0, -1.5, 2.0]).all()
    # lights: 13's ninth is the only one that faces the wall's front (normal -y)
    lights = _world_rows(rec, 13, "lights", "light_counts").view(LIGHT_DT).ravel()
    assert (lights["direction"][:8, 1] < 0).all() and lights["direction"][8, 1] > 0.5
    assert (_world_rows(rec, 12, "lights", "light_counts").view(LIGHT_DT)["direction"]
            .reshape(-1, 3)[:, 1] > 0).all()
    spots = _world_rows(rec, 14, "lights", "light_counts").view(LIGHT_DT).ravel()
    assert (spots["type"] == 0).all() and spots["cutoff"].tolist()[1] == -1.0
    assert spots["castShadow"].tolist() == [0, 0, 1]
    for kind in (4, 5, 6, 8):
        sun = _world_rows(rec, kind, "lights", "light_counts").view(LIGHT_DT).ravel()
        assert sun["type"].tolist() == [1] and sun["castShadow"].tolist() == [1]


def test_equal_codes_and_the_deep_tree():
    rec, geo = _records()
    codes = _world_rows(rec, 7, "codes")
    assert len(codes) == 17 and len(set(codes.tolist())) == 1
    blas = U.median_split_stack_need(int(geo.triangle_offsets[2] - geo.triangle_offsets[1]))
    assert blas >= 4

    deep = _world_rows(rec, 8, "codes")
    assert len(deep) > 64      # not staged in LDS: primary rays walk the tree too
    pairs = (len(deep) - U.DEEP_FILLERS) // 2
    assert sorted(deep.tolist()) == sorted(
        [(1 << (29 - k)) | odd for k in range(pairs) for odd in (0, 1)] +
        [(3 << 28) | j for j in range(2, 2 + U.DEEP_FILLERS)])
    pos = _world_rows(rec, 8).view(INSTANCE_DT)["position"].reshape(-1, 3)
    assert np.ptp(pos, axis=0).max() < 1e-3
    need = U.worst_stack_need(U.karras_children(np.sort(deep)))
    assert need >= 16, need
    assert need + blas <= U.STACK_DEPTH, (need, blas)
    # the innermost instances (the lowest codes) are ellipsoids
    inst = _world_rows(rec, 8).view(INSTANCE_DT).ravel()
    by_code = {}
    for i in inst:
        p = i["position"].view(np.uint32) & 1023
        by_code[int(sum(((int(p[a]) >> b) & 1) << (3 * b + a)
                        for a in range(3) for b in range(10)))] = int(i["objectID"])
    assert [by_code[c] for c in sorted(by_code)[:4]] == [1, 1, 1, 1]

    too_deep, _ = _records(1 << 5)
    assert too_deep["inst_counts"].tolist() == [
        U.TOO_DEEP_INSTANCES if k == 8 else n for k, n in enumerate(U.INSTANCE_COUNTS)]
    need = U.worst_stack_need(U.karras_children(np.sort(_world_rows(too_deep, 8, "codes"))))
    assert need > U.STACK_DEPTH, need


def test_golden_fixture_is_current():
    rec, _ = _records()
    gold = np.load(U.GOLDEN)
    assert sorted(gold.files) == sorted(rec)
    for key in rec:
        assert np.array_equal(gold[key], rec[key]), key


@pytest.mark.parametrize("res", [32, 33, 17, 8, 1])
def test_few_pixels_are_undecided(res):
    """(17: the GPU test's partial-tile resolution, held to the same 3 %)"""
    depth, _, decided, _, _ = _f64(res)
    per_view, per_kind = U.undecided_caps(res)
    for kind in range(U.KINDS):
        d = decided[2 * kind:2 * kind + 2]
        assert (~d).sum() <= per_kind and ((~d).sum((1, 2)) <= per_view).all(), \
            (res, kind, int((~d).sum()))
        if kind >= 1 and res >= 32:
            assert (depth[2 * kind:2 * kind + 2] > 0).mean() > 0.10, (res, kind)


@pytest.mark.parametrize("res", [32, 33])
def test_every_kind_shows_what_it_is_for(res):
    rec, geo = _records()
    depth, rgb, decided, states, hit_inst = _f64(res)

    def seen(kind, state):
        return sum(int(((states[v] == state).any(-1) & decided[v]).sum())
                   for v in (2 * kind, 2 * kind + 1))

    for kind in (4, 5, 6, 8, 14):
        assert seen(kind, F.SHADOWED) >= 20 and seen(kind, F.LIT) >= 20, \
            (res, kind, seen(kind, F.SHADOWED), seen(kind, F.LIT))
    assert seen(14, F.OUT_OF_CONE) >= 20
    # both sides of the first lamp's cone, the one without a cone lights all
    cone = np.concatenate([states[v][decided[v] & (depth[v] > 0)] for v in (28, 29)])
    assert (cone[:, 0] == F.LIT).sum() >= 20 and (cone[:, 0] == F.OUT_OF_CONE).sum() >= 20
    assert (cone[:, 1] == F.LIT).all()

    # 13: dropping the ninth light moves the wall's front by many steps
    without = _f64(res, drop_light=8, worlds=(13,))[1]
    fall = (rgb[26:28][..., :3].astype(int) - without[..., :3].astype(int)).max(-1)
    assert ((fall > 10) & decided[26:28]).sum() >= 100, int(((fall > 10) & decided[26:28]).sum())

    # 9: viewer 0 sits inside a box, sees none of it and what lies beyond it
    inst = _world_rows(rec, 9).view(INSTANCE_DT).ravel()
    around = int(np.flatnonzero((inst["position"] == [0, 0, 1.5]).all(1))[0])
    behind = int(np.flatnonzero(inst["position"][:, 1] < -5)[0])
    lo, hi = inst["position"][around] - 1, inst["position"][around] + 1
    eye = rec["views"].view(VIEW_DT).ravel()[18]["position"]
    assert (eye > lo).all() and (eye < hi).all()
    v0 = hit_inst[18]
    assert (v0 != around).all()
    for beyond in np.flatnonzero(inst["position"][:, 1] > 5):
        assert ((v0 == beyond) & decided[18]).sum() >= 20, (res, int(beyond))
    assert (hit_inst[18:20] != behind).all()
    # the floor runs from behind both cameras to far in front of them
    floor = int(np.flatnonzero(inst["scale"][:, 1] > 20)[0])
    assert inst["position"][floor, 1] - inst["scale"][floor, 1] / 2 < -5
    assert (hit_inst[18:20] == floor).sum() >= 100

    # 10: box tops at exactly viewer 0's height
    tops = _world_rows(rec, 10).view(INSTANCE_DT).ravel()
    assert ((tops["position"][:, 2] + tops["scale"][:, 2] / 2) == 1.5).sum() == 3
    assert (tops["rotation"] == [1, 0, 0, 0]).all()


def _oracle_images(res):
    """ref_render on the same records (worlds without instances left out: the
    reference's kernel reads a root node for every view's world)."""
    rec, geo = _records()
    ic, lc = rec["inst_counts"], rec["light_counts"]
    keep = np.flatnonzero(ic > 0)
    new_index = -np.ones(U.KINDS, np.int64)
    new_index[keep] = np.arange(len(keep))
    views = rec["views"].view(VIEW_DT).ravel().copy()
    kept = new_index[views["worldIDX"]] >= 0
    v = views[kept]
    v["worldIDX"] = new_index[v["worldIDX"]]
    lights = np.concatenate([_world_rows(rec, w, "lights", "light_counts") for w in keep])

    def offsets(counts):
        return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)

    rgb, depth = ref_render(geo, len(keep), rec["instances"], offsets(ic[keep]), ic[keep], v,
                            lights, offsets(lc[keep]), lc[keep], res,
                            threads=min(16, os.cpu_count() or 1))
    return kept, rgb, depth


@pytest.mark.parametrize("res", [32, 33])
def test_the_oracle_is_pinned_by_the_same_definition(res):
    w_depth, w_rgb, decided, _, _ = _f64(res)
    kept, rgb, depth = _oracle_images(res)
    w_depth, w_rgb, decided = w_depth[kept], w_rgb[kept], decided[kept]
    hit, w_hit = depth > 0, w_depth > 0
    assert not ((hit != w_hit) & decided).any()
    both = decided & w_hit
    rel = np.abs(depth[both] - w_depth[both]) / w_depth[both]
    diff = np.abs(rgb[..., :3].astype(int) - w_rgb[..., :3].astype(int)).max(-1)[both]
    print(f"oracle against float64, res {res}: largest relative depth error "
          f"{rel.max():.3e}, pixels one step off {(diff == 1).sum()}, beyond {(diff > 1).sum()}")
    assert rel.max() <= U.ORACLE_DEPTH_ERROR, float(rel.max())
    assert U.DEPTH_RTOL == 2 * U.ORACLE_DEPTH_ERROR and U.COLOUR_STEPS == 1
    assert (diff > 1).sum() == 0
    assert (rgb[..., 3] == 255).all() and (rgb[~hit][:, :3] == 0).all()
