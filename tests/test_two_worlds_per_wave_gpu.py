"""Two worlds per wavefront in the wave box queries
(findFirstEntitiesWithinAABBsWave<.., 32>): the systems that ask them run 32
lanes per world, so half h of a wavefront answers for world 2p + h.  What can go
wrong is the pairing -- an empty half behind an odd world count, halves whose
worlds ask different numbers of boxes or none, a half whose tree has a rebuild
pending while the other's has not -- so the shapes are the smallest that have
those, in lock step with the reference CPU backend, every dumped column bit for
bit.  The 64-lane instantiation (ball_pit) is checked on trees of more leaves
than lanes."""
import os

import numpy as np
import pytest

from madrona_amd.simlib import Simulator, hip_lib_path, ref_lib_path
from parity_utils import compare_columns, run_pair

pytestmark = pytest.mark.gpu


def _need_ref(sim):
    if not os.path.exists(ref_lib_path(sim)):
        pytest.skip("oracle/_ref missing on this box")


def _actions(seed, agents):
    """A new random action set every step; the last component is the grab
    (Escape Room) / lock (Hide-and-Seek) button."""
    rng = np.random.default_rng(seed)

    def feed(ref, hip, step):
        shape = (ref.num_worlds, agents)
        a = np.stack([rng.integers(0, 4, shape), rng.integers(0, 8, shape),
                      rng.integers(-2, 3, shape), rng.integers(0, 2, shape)],
                     -1).astype(np.int32)
        ref.write_tensor("action", a)
        hip.write_tensor("action", a)
    return feed


@pytest.mark.parametrize("denom", [3, 40])
@pytest.mark.parametrize("worlds", [1, 2, 3, 65])
def test_escape_room_phys_pairs(built, worlds, denom):
    """28 leaves per world.  1, 3 and 65 worlds end on a pair with an empty
    half.  Auto-reset 1 in 3: most steps have pairs where one half, both or
    neither was just reset; 1 in 40: few.  grab = 1 half of the time: the
    32-lane grab queries run with 0, 1 or 2 boxes per half, attach and
    release."""
    _need_ref("escape_room_phys")
    probs, step = run_pair("escape_room_phys", worlds, 40, flags=denom,
                           actions=_actions(100 + worlds, 2), check_init=False)
    assert not probs, (step, probs[:3])


@pytest.mark.parametrize("worlds", [3, 16])
def test_hideseek_pairs(built, worlds):
    """29 leaves per world; the lock system's box queries (up to five boxes
    per world) run 32 lanes per world as well."""
    _need_ref("hideseek")
    probs, step = run_pair("hideseek", worlds, 40, flags=5,
                           actions=_actions(200 + worlds, 5), check_init=False)
    assert not probs, (step, probs[:3])


def test_ball_pit_crowd_keeps_64_lane_queries(built, monkeypatch):
    """ball_pit, crowd mode 140: 159 leaves per world; its four box queries per
    world stay 64 lanes wide (three windows of 64 leaves).  Budgets and seed of
    test_ball_pit_wave_box_queries; no resets."""
    _need_ref("ball_pit")
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CANDIDATES_PER_WORLD", "2048")
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CONTACTS_PER_WORLD", "1024")
    worlds, steps, flags = 16, 30, 140 << 16
    with Simulator(ref_lib_path("ball_pit"), worlds, seed=5, flags=flags,
                   num_workers=1) as ref, \
            Simulator(hip_lib_path("ball_pit"), worlds, seed=5, flags=flags) as hip:
        for step in range(1, steps + 1):
            ref.step(1)
            hip.step(1)
            if step % 10 == 0:
                r, h = ref.read_tensor("query_probe"), hip.read_tensor("query_probe")
                assert np.array_equal(r, h), (step, np.flatnonzero((r != h).any(1))[:5])
        assert not compare_columns(ref.dump_all(), hip.dump_all())
        assert (hip.read_tensor("query_probe")[:, 1] > steps).all()
