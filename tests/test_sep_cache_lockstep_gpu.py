"""The LDS physics step remembers, per hull-hull candidate and for one step, the
face that separated the pair, and tries that face alone in the next substep
(DESIGN.md 16.10).  The entry lives beside the candidate list of the world's
LDS block, is written by the lane that owns the candidate -- for a pair the
other half of the wavefront tested, out of the outcome word that crosses the
halves -- and dies with the step.  What can go wrong is the bookkeeping: an
entry that survives into another candidate list, a half that reads its
neighbour's entries, a world that leaves for the HBM step in the middle of a
step.  So: the smallest world counts that have an empty half, a full
wavefront, an odd count and more than one wavefront, in lock step with the
reference CPU backend, every dumped column bit for bit after every step; then
the same with the block's contact capacity cut, so that worlds bail out to the
HBM step between substeps with entries in place.

No simulator flag forces "one world of a wavefront has two or more hull-hull
pairs and the other none" (the pair that is then stolen): which world touches
what follows from the random actions, and nothing here asserts that a pair was
stolen.  The widened outcome word is pinned by tests/test_sep_cache_gpu.py."""
import os

import numpy as np
import pytest

from madrona_amd.simlib import ref_lib_path
from parity_utils import run_pair

pytestmark = pytest.mark.gpu

# (escape_room_phys: 2 agents per world, auto-reset 1 in 40; hideseek: 5, flags 5)
SIMS = {"escape_room_phys": (2, 40), "hideseek": (5, 5)}


def _need_ref(sim):
    if not os.path.exists(ref_lib_path(sim)):
        pytest.skip("oracle/_ref missing on this box")


def _actions(seed, agents):
    rng = np.random.default_rng(seed)

    def feed(ref, hip, step):
        shape = (ref.num_worlds, agents)
        a = np.stack([rng.integers(0, 4, shape), rng.integers(0, 8, shape),
                      rng.integers(-2, 3, shape), rng.integers(0, 2, shape)],
                     -1).astype(np.int32)
        ref.write_tensor("action", a)
        hip.write_tensor("action", a)
    return feed


@pytest.mark.parametrize("worlds", [1, 2, 3, 65])
@pytest.mark.parametrize("sim", sorted(SIMS))
def test_lockstep(built, sim, worlds):
    _need_ref(sim)
    agents, flags = SIMS[sim]
    probs, step = run_pair(sim, worlds, 40, flags=flags,
                           actions=_actions(300 + worlds, agents), check_init=False)
    assert not probs, (step, probs[:3])


@pytest.mark.parametrize("cap", ["6", "12"])
@pytest.mark.parametrize("worlds", [1, 2, 3, 65])
@pytest.mark.parametrize("sim", sorted(SIMS))
def test_lockstep_with_worlds_bailing_out(built, monkeypatch, sim, worlds, cap):
    """The Escape Room holds about 14 contacts per world and substep
    (step_lds.inl, WorldBlock): with room for 12 a world leaves for the HBM
    step in whichever substep first has more -- the first or a later one,
    behind substeps that left entries --, with room for 6 in the first."""
    _need_ref(sim)
    monkeypatch.setenv("MADRONA_MWHIP_PHYS_LDS_CONTACTS", cap)
    agents, flags = SIMS[sim]
    probs, step = run_pair(sim, worlds, 40, flags=flags,
                           actions=_actions(400 + worlds, agents), check_init=False)
    assert not probs, (step, probs[:3])
