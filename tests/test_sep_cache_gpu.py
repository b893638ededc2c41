"""The remembered separating face of a hull-hull candidate, function by function
ON THE DEVICE (``pytest -m gpu``; tests/shims/sep_cache_device_shim.hip ->
libsep_cache_device_test.so).

The LDS physics step keeps, per hull-hull candidate and for one step, the face
that separated the pair when it was last tested, and tries that face alone, on
one lane, before the cooperative test.  That is exact only if

* the one lane computes for face f the very distance the cooperative face query
  computes for it from the hulls staged in LDS -- as bits;
* a candidate with ANY entry -- the right one, a stale one, one that names no
  face -- ends with the contact and the has-contact flag of a candidate without
  one, which are those of the reference's narrowphase (oracle/_ref/
  libphys_ref.so, the entry point of tests/test_physics_functions_gpu.py);
* an entry is left behind exactly when a face with index < 16 of hulls that fit
  the LDS scratch separated the pair: not after an overlap, not after a
  separation along an edge axis, not for hulls beyond the scratch.

Pairs of the Escape Room's box hull and of Hide-and-Seek's wedge ramp (and of a
16-sided prism that does not fit the scratch), rotated and scaled: separated by
a face of A, by a face of B only, along an edge axis only, overlapping, and
touching with a separation of exactly 0.0f, which must not count as separated."""
import ctypes as C
import os

import numpy as np
import pytest

from madrona_amd.simlib import HIP_BUILD_DIR, REF_BUILD_DIR
from test_physics_functions import MESHES, _ptr, _random_quat

pytestmark = pytest.mark.gpu

DEV = os.path.join(HIP_BUILD_DIR, "libsep_cache_device_test.so")
REF = os.path.join(REF_BUILD_DIR, "libphys_ref.so")

FACES = 16                  # sepFaceLimit
OF_A, OF_B = 0x10, 0x20     # sepFaceOfA, sepFaceOfB
# a candidate without an entry, every entry that can name a face, and bytes that
# name none: both hulls at once, neither, bits beyond the entry
ENTRIES = np.array([0] + [OF_A | f for f in range(FACES)] +
                   [OF_B | f for f in range(FACES)] +
                   [0x30, 0x3F, 0x05, 0x0F, 0x40, 0x91, 0xFF], np.uint8)


def _random_pairs(rng, n):
    """Hulls of 0.6 to 1.8 times the mesh's size, any orientation, centres 0.4
    to 2.6 apart: about half overlap, the rest are apart by a face or an edge."""
    out = np.zeros((n, 20), np.float32)
    for t in range(n):
        tilt = 0.05 if t % 4 == 0 else np.pi
        a = np.concatenate([rng.uniform(-1, 1, 3), _random_quat(rng, tilt),
                            rng.uniform(0.6, 1.8, 3)])
        d = rng.normal(size=3)
        d *= rng.uniform(0.4, 2.6) / np.linalg.norm(d)
        b = np.concatenate([a[:3] + d, _random_quat(rng, tilt),
                            rng.uniform(0.6, 1.8, 3)])
        out[t, :10], out[t, 10:] = a, b
    return out


def _touching_pairs():
    """Cubes (corners at +-0.5) whose faces meet with a separation of exactly
    0.0f: scales that are powers of two, centres on a grid of 1/8, and turns
    of 0 or 180 degrees about an axis, whose rotation matrices are exact."""
    turns = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    out = []
    for qa in turns:
        for qb in turns:
            for sa, sb, axis in [([2, 1, 4], [1, 2, .5], 0), ([.5, 4, 1], [2, 2, 1], 1),
                                 ([1, 1, 2], [4, .5, 2], 2)]:
                centre = np.array([.125, -.25, .375])
                off = np.array([.25, -.125, .125])
                off[axis] = (sa[axis] + sb[axis]) / 2
                for sign in (1, -1):
                    out.append(np.concatenate([centre, qa, sa,
                                               centre + sign * off, qb, sb]))
    return np.array(out, np.float32)


@pytest.fixture(scope="module")
def libs(built):
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref missing on this box")
    import torch  # noqa: F401  (torch's HIP runtime first, see simlib)
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    dev, ref = C.CDLL(DEV), C.CDLL(REF)
    mesh_args = [C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32),
                 C.POINTER(C.c_uint32), C.c_uint32]
    ref.ref_collide_pair.argtypes = mesh_args + [
        C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_float)]
    dev.dev_sep_cache_pairs.restype = C.c_int32
    dev.dev_sep_cache_pairs.argtypes = mesh_args + [
        C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32,
        C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
        C.POINTER(C.c_int32)]
    return dev, ref


def _run(libs, mesh, pairs):
    """(reference contacts, one-lane distances, cooperative distances, contacts
    and flags per entry of ENTRIES) of `pairs` of `mesh`."""
    dev, ref = libs
    verts, idx, counts = MESHES[mesh]
    n, trials = len(pairs), len(ENTRIES)
    mesh_args = (_ptr(verts, C.c_float), len(verts), _ptr(idx, C.c_uint32),
                 _ptr(counts, C.c_uint32), len(counts))

    expect = np.zeros((n, 28), np.float32)
    for t in range(n):
        a, b = pairs[t, :10].copy(), pairs[t, 10:].copy()
        ref.ref_collide_pair(*mesh_args, _ptr(a, C.c_float), _ptr(b, C.c_float), 0,
                             _ptr(expect[t], C.c_float))

    entries = np.ascontiguousarray(np.tile(ENTRIES, (n, 1)))
    lane = np.zeros((n, 2, FACES), np.float32)
    coop = np.zeros((n, 2, FACES), np.float32)
    got = np.zeros((n, trials, 28), np.float32)
    flags = np.zeros((n, trials), np.int32)
    rc = dev.dev_sep_cache_pairs(*mesh_args, _ptr(pairs, C.c_float), n,
                                 _ptr(entries, C.c_uint8), trials,
                                 _ptr(lane, C.c_float), _ptr(coop, C.c_float),
                                 _ptr(got, C.c_float), _ptr(flags, C.c_int32))
    assert rc == 0
    return expect, lane, coop, got, flags


def _face_query(dist):
    """(separation, face) of queryFaceDirectionsWave over per-face distances:
    the maximum, the first face that reaches it; a NaN never wins."""
    best, face = -np.inf, -1
    for f, d in enumerate(dist):
        if d > best:
            best, face = d, f
    return best, face


def _entry_after_test(dist_a, dist_b):
    """What hullHullWaveSAT reports for hulls that fit the scratch."""
    sep, face = _face_query(dist_a)
    if sep > 0:
        return OF_A | face if face < FACES else 0
    sep, face = _face_query(dist_b)
    if sep > 0:
        return OF_B | face if face < FACES else 0
    return 0


def _check(mesh, pairs, expect, lane, coop, got, flags):
    """Every property above for every pair; returns the pairs by class."""
    num_faces = len(MESHES[mesh][2])
    fits = num_faces <= FACES and len(MESHES[mesh][0]) <= FACES
    classes = {k: [] for k in ("face_a", "face_b", "edge", "overlap", "touching")}

    for t in range(len(pairs)):
        where = (mesh, t, pairs[t])
        # the one-lane distance of every face is the cooperative query's
        shown = min(num_faces, FACES)
        assert not np.isnan(lane[t, :, :shown]).any(), where
        assert np.isnan(lane[t, :, shown:]).all(), where
        if fits:
            assert np.array_equal(lane[t].view(np.uint32), coop[t].view(np.uint32)), \
                (where, lane[t], coop[t])
        else:
            assert np.isnan(coop[t]).all(), where

        # a candidate without an entry: the reference's contact
        base_flags = int(flags[t, 0])
        assert not base_flags & 4, where
        assert bool(base_flags & 2) == (not fits), where
        used = 6 + 4 * int(expect[t, 2])    # (the slots the reference fills)
        if not base_flags & 1:      # (too big: the step kernel reruns the pair in HBM)
            assert np.array_equal(expect[t, :used].view(np.uint32),
                                  got[t, 0, :used].view(np.uint32)), \
                (where, expect[t, :used], got[t, 0, :used])

        # ... and the entry it is left with
        want_entry = _entry_after_test(lane[t, 0, :shown], lane[t, 1, :shown]) \
            if fits else 0
        assert base_flags >> 8 == want_entry, (where, base_flags, want_entry)
        if base_flags & 1 or expect[t, 0] != 0:
            assert want_entry == 0, where

        # any entry: the same contact, the same flags; the named face settles
        # the pair exactly when its distance is above zero
        for k, entry in enumerate(ENTRIES):
            entry = int(entry)
            f = entry & (FACES - 1)
            names_face = (entry & ~(FACES - 1)) in (OF_A, OF_B) and f < num_faces
            settles = names_face and lane[t, 0 if entry & OF_A else 1, f] > 0
            assert bool(flags[t, k] & 4) == bool(settles), (where, hex(entry))
            assert (flags[t, k] & 3) == (0 if settles else base_flags & 3), \
                (where, hex(entry))
            assert flags[t, k] >> 8 == (entry if settles else want_entry), \
                (where, hex(entry), flags[t, k])
            assert np.array_equal(got[t, k, :used].view(np.uint32),
                                  got[t, 0, :used].view(np.uint32)), (where, hex(entry))
            if settles:
                assert expect[t, 0] == 0 and not base_flags & 1, (where, hex(entry))

        sep_a = _face_query(lane[t, 0, :shown])[0]
        sep_b = _face_query(lane[t, 1, :shown])[0]
        if sep_a > 0:
            classes["face_a"].append(t)
        elif sep_b > 0:
            classes["face_b"].append(t)
        elif expect[t, 0] == 0 and not base_flags & 1:
            classes["edge"].append(t)
        else:
            classes["overlap"].append(t)
        if max(sep_a, sep_b) == 0:
            classes["touching"].append(t)
    return classes


@pytest.mark.parametrize("mesh", ["cube", "wedge", "coin16"])
def test_any_entry_leaves_the_result_alone(libs, mesh):
    pairs = _random_pairs(np.random.default_rng(700 + len(mesh)), 320)
    classes = _check(mesh, pairs, *_run(libs, mesh, pairs))
    # (every kind of pair is there, rotated and scaled; an edge axis alone
    # separates few: 2 % of the tests of an Escape-Room step)
    counts = {k: len(v) for k, v in classes.items()}
    assert counts["face_a"] >= 30 and counts["overlap"] >= 30, counts
    if mesh != "coin16":
        assert counts["face_b"] >= 8 and counts["edge"] >= 3, counts


def test_touching_is_not_separated(libs):
    """Separation exactly 0.0f: the face query says "not separated" (> 0), so
    must the remembered face -- the pair goes on to the cooperative test, which
    finds the contact or not as the reference does."""
    pairs = _touching_pairs()
    expect, lane, coop, got, flags = _run(libs, "cube", pairs)
    classes = _check("cube", pairs, expect, lane, coop, got, flags)
    assert len(classes["touching"]) == len(pairs) == 96, \
        {k: len(v) for k, v in classes.items()}
    # (the face that touches is remembered by no one, and settles nothing)
    for t in range(len(pairs)):
        for which in (0, 1):
            for f in np.flatnonzero(lane[t, which, :6] == 0):
                k = 1 + which * FACES + int(f)
                assert ENTRIES[k] == (OF_A, OF_B)[which] | f
                assert not flags[t, k] & 4, (t, which, f)
