"""-m gpu: the navmesh_agents simulator (sims/navmesh_agents) in lock step with
the numpy restatement (tests/navmesh_restate.py): every dumped column equal
bit for bit after 1, 7 and 40 steps.  Each world's polygons are read from the
simulator library itself (sim_navmesh_polygons).

Also: what the world constructors take from the executor's persistent region
is the navmeshes' output blocks and nothing else
(mwhip_persist_bytes_used).
"""
import ctypes as C

import numpy as np
import pytest

import navmesh_restate as R
from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib

pytestmark = pytest.mark.gpu

CHECKPOINTS = (1, 7, 40)


def _compare(sim, rest, worlds, step):
    dump = sim.dump_all()
    sel = np.concatenate([np.arange(w * R.AGENTS_PER_WORLD, (w + 1) * R.AGENTS_PER_WORLD)
                          for w in worlds])
    for name, want in rest.columns().items():
        rows, counts = dump[name]
        assert (counts == R.AGENTS_PER_WORLD).all(), name
        got = rows.view(np.uint32).reshape(len(rows), -1)[sel]
        bad = np.nonzero((got != want).any(1))[0]
        assert len(bad) == 0, (step, name, sel[bad[:4]], got[bad[:4]], want[bad[:4]])


@pytest.mark.parametrize("num_worlds", [1, 33, 1024, 8192])
def test_agents_lock_step(built, num_worlds):
    seed, flags = 5, 0
    worlds = list(range(num_worlds))
    with Simulator(hip_lib_path("navmesh_agents"), num_worlds, seed=seed,
                   flags=flags) as sim:
        rest = R.AgentsRestatement(R.Rand(), sim.lib, worlds, seed, flags)
        assert len(set(rest.families)) == min(5, len(worlds))
        for step in range(1, max(CHECKPOINTS) + 1):
            sim.step(1)
            rest.step()
            if step in CHECKPOINTS:
                _compare(sim, rest, worlds, step)


@pytest.mark.parametrize("flags", [0, 2])
def test_persistent_memory_per_world(built, flags):
    num_worlds, seed = 257, 3
    with Simulator(hip_lib_path("navmesh_agents"), num_worlds, seed=seed,
                   flags=flags) as sim:
        lib = runtime_lib()
        lib.mwhip_persist_bytes_used.restype = C.c_uint64
        lib.mwhip_persist_bytes_used.argtypes = [C.c_void_p]
        used = lib.mwhip_persist_bytes_used(C.c_void_p(sim.hip_exec()))
        want = 0
        for w in range(num_worlds):
            _, v, i, o, s = R.agents_polygons(sim.lib, w, seed, flags)
            want += R.device_block_bytes(len(v), int((s - 2).sum()))
        assert used == want
