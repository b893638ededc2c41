"""CPU-only: the float32 restatements of Vector3::normalize and Quat::rotateVec
in madrona_amd/ray_ref.py against <madrona/math.hpp> compiled for the host with
the product's flags (tests/shims/ray_dir_shim.cpp), bit for bit.  The device
tests of the ray queries build their directions from the restatement: the 32
directions of broadphase_only's fanDirection and the 30 lidar directions of
escape_room_phys under the agents' rotations."""
import ctypes as C
import os

import numpy as np

from madrona_amd import ray_ref
from madrona_amd.simlib import HIP_BUILD_DIR
from ray_utils import lidar_table


def _lib():
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libray_dir_host_test.so"))
    F = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    lib.raydir_normalize.argtypes = [F, F, C.c_int32]
    lib.raydir_normalize.restype = None
    lib.raydir_rotate_normalize.argtypes = [F, C.c_int32, F, C.c_int32, F]
    lib.raydir_rotate_normalize.restype = None
    return lib


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


def test_normalize_over_the_fan_direction_inputs(built):
    lib = _lib()
    for plan_mode in (False, True):
        inputs = ray_ref.fan_direction_inputs(plan_mode)
        want = np.empty_like(inputs)
        lib.raydir_normalize(inputs, want, 32)
        _same_bits(ray_ref.normalize_f32(inputs), want, ("normalize", plan_mode))
    # the fan itself: plan mode keeps its five axis-aligned rays as they are
    fan = ray_ref.fan_directions(True)
    assert fan[:5].tolist() == [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, -1]]
    _same_bits(fan[5:], ray_ref.fan_directions(False)[5:], "the rest of the fan")
    assert np.allclose(np.linalg.norm(ray_ref.fan_directions(False), axis=1), 1, atol=1e-6)


def test_rotate_then_normalize_over_the_lidar_table(built):
    lib = _lib()
    table = lidar_table()
    rng = np.random.default_rng(33)
    quats = rng.normal(size=(300, 4)).astype(np.float32)
    quats /= np.linalg.norm(quats, axis=1, keepdims=True).astype(np.float32)
    # ... and the rotations agents really have: about z, identity included
    yaw = rng.uniform(-np.pi, np.pi, 60).astype(np.float32)
    about_z = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], -1).astype(np.float32)
    quats = np.ascontiguousarray(np.concatenate([quats, about_z, [[1, 0, 0, 0]]]).astype(np.float32))
    want = np.empty((len(quats), 30, 3), np.float32)
    lib.raydir_rotate_normalize(quats, len(quats), table, 30, want)
    got = ray_ref.normalize_f32(ray_ref.rotate_vec_f32(quats[:, None, :], table[None, :, :]))
    _same_bits(got, want, "rotateVec + normalize")
    assert np.isfinite(want).all()
