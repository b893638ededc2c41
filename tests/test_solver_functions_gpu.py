"""Function-level parity of the XPBD solver ON THE DEVICE
(tests/shims/phys_device_shim.hip) against the reference's own solver phases
(oracle/_ref/libxpbd_ref.so), over the families of tests/solver_utils.py, bit
for bit:

* mode 0: the scalar routines of phys_impl/xpbd.hpp, one lane per world, every
  combination of phases;
* modes 1-3: the LDS step kernel's own solve (phys_impl/step_solve.inl, two
  lanes per constraint, level by level) over a real WorldBlock / LdsBodyStore,
  as <64, 64>, <32, 32> (two worlds per wavefront) and <128, 64>;
* constraintLevels<LPW> against the greedy rule restated in numpy, and
  wave::nthSetBit<LPW> against Python.
"""
import ctypes as C
import os

import numpy as np
import pytest

from madrona_amd.simlib import HIP_BUILD_DIR, REF_BUILD_DIR

import solver_utils as su

pytestmark = pytest.mark.gpu

DEV = os.path.join(HIP_BUILD_DIR, "libphys_device_test.so")
REF = os.path.join(REF_BUILD_DIR, "libxpbd_ref.so")

FAMILIES = ("pairs", "geometry", "velocity", "joints", "levels", "asymmetric",
            "random")
SOLVE = 30      # contacts, joints, velocities, velocity solve: the kernel's solve

# what each instantiation's block holds: lanes per world, contacts
# (WorldBlock::maxContacts), bodies the solver can change (maxSolverBodies)
BLOCKS = {1: (64, 80, su.MAX_BODIES), 2: (32, 32, 20), 3: (64, None, su.MAX_BODIES)}


@pytest.fixture(scope="module")
def libs(built):
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref not built here (no /root/reference)")
    dev, ref = C.CDLL(DEV), C.CDLL(REF)
    dev.dev_constraint_levels.restype = C.c_int32
    dev.dev_constraint_levels.argtypes = [
        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
        C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    dev.dev_nth_set_bit.restype = C.c_int32
    dev.dev_nth_set_bit.argtypes = [C.POINTER(C.c_uint64), C.c_uint32,
                                    C.c_uint32, C.POINTER(C.c_uint32)]
    su.bind_dev_solve(dev.dev_solve_worlds)
    return dev, su.bind_solve(ref.ref_solve_world)


@pytest.fixture(scope="module")
def family_sets():
    """mode -> families within what that mode's block holds (mode 0: no cap)."""
    sets = {mode: su.all_families(*caps) for mode, caps in BLOCKS.items()}
    sets[0] = sets[3]
    return sets


def _check(worlds, expected, got, what):
    assert len(expected) == len(got) == len(worlds)
    for i, (w, (state, lambdas), (got_state, got_lambdas)) in enumerate(
            zip(worlds, expected, got)):
        # the conditions that hold for the reference alone
        assert np.isfinite(state).all() and np.isfinite(lambdas).all(), w.tag
        assert np.array_equal(state.view(np.uint32),
                              got_state.view(np.uint32)), \
            (what, w.tag, i, np.argwhere(state.view(np.uint32) !=
                                         got_state.view(np.uint32))[:8])
        assert np.array_equal(lambdas.view(np.uint32),
                              got_lambdas.view(np.uint32)), (what, w.tag, i)


@pytest.mark.parametrize("family", FAMILIES)
def test_scalar_solver_on_device_matches_reference(libs, family_sets, family):
    dev, ref = libs
    worlds = family_sets[0][family]
    for w in worlds:
        su.check_input_conditions(w)
    packed = su.Packed(worlds)
    for mask in su.ALL_MASKS:
        expected = [su.solve(ref, w, mask) for w in worlds]
        got = su.dev_solve(dev.dev_solve_worlds, packed, mask, 0)
        _check(worlds, expected, got, ("mode 0", mask))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_kernel_solve_matches_reference(libs, family_sets, mode, family):
    dev, ref = libs
    worlds = family_sets[mode][family]
    for w in worlds:
        su.check_input_conditions(w)
    expected = [su.solve(ref, w, SOLVE) for w in worlds]
    got = su.dev_solve(dev.dev_solve_worlds, su.Packed(worlds), SOLVE, mode)
    _check(worlds, expected, got, ("mode", mode))


def test_kernel_families_reach_their_paths(family_sets):
    """By construction: the windows, rounds and halves the modes must reach."""
    # <64, 64>: a second contact window (65 of 80), a full first one
    counts = {len(w.contacts) for w in family_sets[1]["levels"]}
    assert {0, 1, 64, 65} <= counts and max(counts) <= 80, counts
    # <128, 64>: a third window, and the velocity solve's recomputed levels
    counts = {len(w.contacts) for w in family_sets[3]["levels"]}
    assert {64, 65, 131} <= counts, counts
    # <32, 32>: exactly the cap, and at most 20 bodies the solver can change
    counts = {len(w.contacts) for w in family_sets[2]["levels"]}
    assert 32 in counts and max(counts) == 32, counts
    for worlds in family_sets[2].values():
        assert max(len(w.bodies) for w in worlds) <= 20
    for mode in (1, 3):
        for worlds in family_sets[mode].values():
            assert max(len(w.bodies) for w in worlds) <= 36
    # a level with more members than teams (a second round): an inert star
    for mode, (lpw, _, _) in BLOCKS.items():
        stars = [w for w in family_sets[mode]["levels"]
                 if "star_inert" in w.tag]
        assert len(stars) >= 14
        assert all(len(w.contacts) == lpw // 2 + 3 for w in stars)
    # joints whose rows are read from HBM (beyond Block::maxJoints = 2), up to
    # Block::maxJointBodies = 8 of them
    joints = {len(w.joints) for w in family_sets[1]["joints"]}
    assert {1, 2, 3, 8} <= joints, joints
    # asymmetric halves: neighbours 2i, 2i + 1 share a wavefront in mode 2
    asym = family_sets[2]["asymmetric"]
    halves = [(len(asym[i].contacts), len(asym[i + 1].contacts),
               len(asym[i].joints), len(asym[i + 1].joints))
              for i in range(0, len(asym), 2)]
    assert sum(1 for a, b, _, _ in halves if {a, b} == {0, 32}) >= 20
    assert sum(1 for a, b, _, _ in halves if {a, b} == {1, 12}) >= 10
    assert sum(1 for _, _, a, b in halves if (a == 0) != (b == 0)) >= 10


# ------------------------------------------------------------------------------
# constraintLevels<LPW>
# ------------------------------------------------------------------------------
def _level_cases(lpw):
    rng = np.random.default_rng(900 + lpw)
    cases = []      # (keys_a, keys_b) of n constraints each
    for n in (0, 1, 2, lpw - 1, lpw):
        # a chain, a star round key 0, disjoint pairs
        cases.append(([1] * n, list(range(2, n + 2))))
        cases.append(([0] * n, list(range(2, n + 2))))
        cases.append((list(range(1, 2 * n, 2)), list(range(2, 2 * n + 1, 2))))
        # a constraint whose two keys are equal, one whose keys are both zero,
        # then a chain through key 9
        cases.append((([7, 7, 8, 0] + [9] * lpw)[:n],
                      ([7, 8, 9, 0] + list(range(10, 10 + lpw)))[:n]))
        # random graphs over few bodies, a third of the keys zero
        for bodies in (3, 8, 40):
            for _ in range(6):
                a = rng.integers(0, bodies + 1, n)
                b = rng.integers(0, bodies + 1, n)
                zero = rng.random(n) < 0.33
                cases.append((list(np.where(zero, 0, a)), list(b)))
    # neighbours with very different counts (lpw 32: the halves of a wavefront)
    cases.sort(key=lambda c: len(c[0]))
    mixed = []
    for i in range(len(cases) // 2):
        mixed += [cases[i], cases[len(cases) - 1 - i]]
    return mixed + ([cases[len(cases) // 2]] if len(cases) % 2 else [])


@pytest.mark.parametrize("lpw", [64, 32])
def test_constraint_levels_match_the_greedy_rule(libs, lpw):
    dev, _ = libs
    cases = _level_cases(lpw)
    assert {len(a) for a, _ in cases} == {0, 1, 2, lpw - 1, lpw}
    keys_a = np.zeros((len(cases), lpw), np.uint32)
    keys_b = np.zeros((len(cases), lpw), np.uint32)
    counts = np.zeros(len(cases), np.uint32)
    want = np.zeros((len(cases), lpw), np.uint32)
    for i, (a, b) in enumerate(cases):
        assert len(a) == len(b)
        keys_a[i, :len(a)], keys_b[i, :len(b)], counts[i] = a, b, len(a)
        want[i, :len(a)] = su.greedy_levels(a, b)
    assert want.max() == lpw - 1        # the chain
    got = np.full((len(cases), lpw), 0xDEAD, np.uint32)
    rc = dev.dev_constraint_levels(su._ptr(keys_a, C.c_uint32),
                                   su._ptr(keys_b, C.c_uint32),
                                   su._ptr(counts, C.c_uint32), len(cases), lpw,
                                   su._ptr(got, C.c_uint32))
    assert rc == 0
    bad = np.argwhere(want != got)
    assert len(bad) == 0, (bad[:8], [cases[i] for i in bad[:2, 0]])


# ------------------------------------------------------------------------------
# wave::nthSetBit<LPW>
# ------------------------------------------------------------------------------
def _bit_masks(lpw):
    rng = np.random.default_rng(1000 + lpw)
    full = (1 << lpw) - 1
    masks = [1 << b for b in range(lpw)]                    # single bits
    masks += [full, full >> 1, full & ~1, 0]                # dense, empty
    masks += [full ^ (1 << b) for b in (0, 15, 16, 31, lpw - 1)]
    masks += [(1 << (lpw - 1)) | 1, 0x80008000 & full, 0xFFFF0000 & full]
    for density in (0.05, 0.5, 0.95):                       # sparse .. dense
        for _ in range(40):
            bits = rng.random(lpw) < density
            masks.append(sum(1 << int(b) for b in np.flatnonzero(bits)))
    return masks


@pytest.mark.parametrize("lpw", [64, 32])
def test_nth_set_bit_matches_python(libs, lpw):
    dev, _ = libs
    masks = _bit_masks(lpw)
    arr = np.array(masks, np.uint64)
    want = np.full((len(masks), 64), 0xFFFFFFFF, np.uint32)
    for i, m in enumerate(masks):
        positions = [b for b in range(64) if (m >> b) & 1]
        want[i, :len(positions)] = positions
    got = np.zeros((len(masks), 64), np.uint32)
    rc = dev.dev_nth_set_bit(su._ptr(arr, C.c_uint64), len(masks), lpw,
                             su._ptr(got, C.c_uint32))
    assert rc == 0
    bad = np.argwhere(want != got)
    assert len(bad) == 0, (bad[:8], [hex(masks[i]) for i in bad[:4, 0]])
