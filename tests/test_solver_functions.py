"""CPU-only, function-level parity of the XPBD solver: the overlay's scalar
solver routines (phys_impl/xpbd.hpp, compiled for the host by
tests/shims/phys_host_shim.cpp: amd_solve_world) against the reference's own
solver phases (oracle/_ref/libxpbd_ref.so: ref_solve_world, the reference's
Context-taking routines over a real StateManager), over the families of
tests/solver_utils.py, for every combination of phases, bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest

from madrona_amd.simlib import HIP_BUILD_DIR, REF_BUILD_DIR

import solver_utils as su

AMD = os.path.join(HIP_BUILD_DIR, "libphys_host_test.so")
REF = os.path.join(REF_BUILD_DIR, "libxpbd_ref.so")

FAMILIES = ("pairs", "geometry", "velocity", "joints", "levels", "asymmetric",
            "random")


@pytest.fixture(scope="module")
def libs(built):
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref not built here (no /root/reference)")
    amd, ref = C.CDLL(AMD), C.CDLL(REF)
    return su.bind_solve(amd.amd_solve_world), su.bind_solve(ref.ref_solve_world)


@pytest.fixture(scope="module")
def families():
    return su.all_families()


@pytest.fixture(scope="module")
def expected(libs, families):
    """The reference's outputs, computed once: family -> [world][mask]."""
    _, ref = libs
    return {name: [{mask: su.solve(ref, w, mask) for mask in su.ALL_MASKS}
                   for w in worlds]
            for name, worlds in families.items()}


@pytest.mark.parametrize("family", FAMILIES)
def test_input_conditions(families, expected, family):
    """What must hold for the reference alone before anything is compared."""
    for w, by_mask in zip(families[family], expected[family]):
        su.check_input_conditions(w)
        for mask, (state, lambdas) in by_mask.items():
            assert np.isfinite(state).all(), (w.tag, mask)
            assert np.isfinite(lambdas).all(), (w.tag, mask)


@pytest.mark.parametrize("family", FAMILIES)
def test_scalar_solver_matches_reference(libs, families, expected, family):
    amd, _ = libs
    compared = 0
    for i, (w, by_mask) in enumerate(zip(families[family], expected[family])):
        for mask, (state, lambdas) in by_mask.items():
            got_state, got_lambdas = su.solve(amd, w, mask)
            assert np.array_equal(state.view(np.uint32),
                                  got_state.view(np.uint32)), \
                (w.tag, i, mask, np.argwhere(state.view(np.uint32) !=
                                             got_state.view(np.uint32))[:8])
            assert np.array_equal(lambdas.view(np.uint32),
                                  got_lambdas.view(np.uint32)), (w.tag, i, mask)
            compared += 1
    assert compared == len(families[family]) * len(su.ALL_MASKS)


POSITION = 2 | 4    # contacts, then joints
POSE = slice(0, 7)


def _tags(worlds, *prefixes):
    return [i for i, w in enumerate(worlds)
            if any(p in w.tag for p in prefixes)]


def test_families_reach_their_branches(families, expected):
    """Coverage, counted from the reference's outputs (and, for the level and
    asymmetric families, from the constructed counts).  The floors are a little
    under what the reference gives here; observed counts beside each."""
    zero = pos = 0
    for name in FAMILIES:
        for w, by_mask in zip(families[name], expected[name]):
            lambdas = by_mask[2][1]
            zero += int((lambdas == 0).sum())
            pos += int((lambdas != 0).sum())
    assert zero >= 900, zero        # observed: 974
    assert pos >= 9000, pos         # observed: 9535

    # a static body that the position solve moved (its rotation renormalised)
    moved = 0
    for name in ("pairs", "levels", "joints", "random"):
        for w, by_mask in zip(families[name], expected[name]):
            state = by_mask[POSITION][0]
            for b in np.flatnonzero(w.types == su.STATIC):
                if not np.array_equal(state[b, POSE].view(np.uint32),
                                      w.bodies[b, POSE].view(np.uint32)):
                    moved += 1
                    break
    # observed: 67 (pairs 20, levels 14, joints 1, random 32)
    assert moved >= 60, moved

    # -0.0 on a static body turned into +0.0 (x1 += 0 * n)
    flipped = 0
    for i in _tags(families["pairs"], "static_neg_zero"):
        w, state = families["pairs"][i], expected["pairs"][i][2][0]
        b = int(np.flatnonzero(w.types == su.STATIC)[0])
        flipped += int((np.signbit(w.bodies[b, 0:3]) &
                        ~np.signbit(state[b, 0:3])).any())
    assert flipped >= 7, flipped    # observed: 8 of 11 worlds

    # worlds whose velocity solve changed nothing / something
    same = changed = 0
    for name in FAMILIES:
        for w, by_mask in zip(families[name], expected[name]):
            if not len(w.contacts):
                continue
            if np.array_equal(by_mask[16][0].view(np.uint32),
                              w.bodies[:, :su.BODY_STATE].view(np.uint32)):
                same += 1
            else:
                changed += 1
    assert same >= 18, same         # observed: 20
    assert changed >= 700, changed  # observed: 761

    # restitution: e = 0 at and below the threshold, 0.3 above
    vel = families["velocity"]
    for kind in ("below", "at", "above", "no_tangential_velocity",
                 "zero_lambda", "unequal_depths"):
        assert len(_tags(vel, "velocity/" + kind)) >= 20, kind

    # joints that left both bodies exactly where they were
    idle = 0
    for i in _tags(families["joints"], "fixed_satisfied"):
        w, state = families["joints"][i], expected["joints"][i][4][0]
        idle += int(np.array_equal(state[:, POSE].view(np.uint32),
                                   w.bodies[:, POSE].view(np.uint32)))
    assert idle >= 10, idle         # observed: 10 of 10

    # constructed counts of the level and asymmetric families
    levels = families["levels"]
    counts = sorted({len(w.contacts) for w in levels})
    assert {0, 1, 64, 65, 131} <= set(counts), counts
    for kind in su.LEVEL_KINDS:
        assert len(_tags(levels, "levels/" + kind + "/")) >= 14, kind
    asym = families["asymmetric"]
    halves = [(len(asym[i].contacts), len(asym[i + 1].contacts),
               len(asym[i].joints), len(asym[i + 1].joints))
              for i in range(0, len(asym), 2)]
    assert sum(1 for a, b, _, _ in halves if {a, b} == {0, 32}) >= 20
    assert sum(1 for _, _, a, b in halves if (a == 0) != (b == 0)) >= 10
    assert sum(1 for a, b, _, _ in halves if {a, b} == {1, 12}) >= 10


# ------------------------------------------------------------------------------
# the greedy level rule, against answers written by hand
# ------------------------------------------------------------------------------
def test_greedy_levels_by_hand():
    # a chain: every constraint shares body 1
    assert su.greedy_levels([1, 1, 1, 1], [2, 3, 4, 5]) == [0, 1, 2, 3]
    # a star round an inert static body (key 0): nothing conflicts
    assert su.greedy_levels([0, 0, 0, 0], [2, 3, 4, 5]) == [0, 0, 0, 0]
    assert su.greedy_levels([2, 0, 4, 0], [0, 3, 0, 5]) == [0, 0, 0, 0]
    # the same star round a body with a key of its own serialises
    assert su.greedy_levels([9, 9, 9], [2, 3, 4]) == [0, 1, 2]
    # disjoint pairs
    assert su.greedy_levels([1, 3, 5], [2, 4, 6]) == [0, 0, 0]
    # the level is one above the HIGHEST earlier conflict, not the latest:
    # (1,2) (2,3) (3,4) are levels 0 1 2; (1,4) conflicts with levels 0 and 2
    assert su.greedy_levels([1, 2, 3, 1], [2, 3, 4, 4]) == [0, 1, 2, 3]
    # ... and a later, lower conflict does not pull it down
    assert su.greedy_levels([1, 2, 5, 2], [2, 3, 6, 5]) == [0, 1, 0, 2]
    # both keys equal; a constraint whose keys are both 0
    assert su.greedy_levels([7, 7, 0], [7, 8, 0]) == [0, 1, 0]
    assert su.greedy_levels([], []) == []
