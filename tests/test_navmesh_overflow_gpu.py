"""-m gpu: navmesh_agents when its world constructors ask for more memory than
the executor's regions hold.

The constructors run before the scratch region can grow on demand, and the
persistent region is sized from MADRONA_MWHIP_PERSIST_KB_PER_WORLD.  When either
overflows, the allocation that did not fit returns the region's base: the
navmesh builder and the simulator then write nothing (an empty mesh), and the
executor sizes the regions from what the pass asked for and runs the
constructors again.  Every dumped column must still equal the numpy
restatement bit for bit, and the persistent region must hold the navmeshes'
output blocks and nothing else.
"""
import ctypes as C

import numpy as np
import pytest

import navmesh_restate as R
from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib

pytestmark = pytest.mark.gpu


def _compare(sim, rest, step):
    dump = sim.dump_all()
    for name, want in rest.columns().items():
        rows, counts = dump[name]
        assert (counts == R.AGENTS_PER_WORLD).all(), name
        got = rows.view(np.uint32).reshape(len(rows), -1)
        bad = np.nonzero((got != want).any(1))[0]
        assert len(bad) == 0, (step, name, bad[:4], got[bad[:4]], want[bad[:4]])


def _persist_used(sim):
    lib = runtime_lib()
    lib.mwhip_persist_bytes_used.restype = C.c_uint64
    lib.mwhip_persist_bytes_used.argtypes = [C.c_void_p]
    return lib.mwhip_persist_bytes_used(C.c_void_p(sim.hip_exec()))


def _lock_step(num_worlds, seed, flags, checkpoints):
    with Simulator(hip_lib_path("navmesh_agents"), num_worlds, seed=seed,
                   flags=flags) as sim:
        rest = R.AgentsRestatement(R.Rand(), sim.lib, range(num_worlds), seed, flags)
        want = sum(R.device_block_bytes(len(v), int((s - 2).sum()))
                   for v, _, _, s in rest.polygons)
        assert _persist_used(sim) == want
        _compare(sim, rest, 0)
        for step in range(1, max(checkpoints) + 1):
            sim.step(1)
            rest.step()
            if step in checkpoints:
                _compare(sim, rest, step)


@pytest.mark.parametrize("env,num_worlds,flags", [
    ({"MADRONA_MWHIP_TMP_MB": "1"}, 1024, 2),
    ({"MADRONA_MWHIP_TMP_MB": "1", "MADRONA_MWHIP_TABLE_GROWTH": "1"}, 257, 2),
    ({"MADRONA_MWHIP_PERSIST_KB_PER_WORLD": "1"}, 1024, 2),
    ({"MADRONA_MWHIP_TMP_MB": "1", "MADRONA_MWHIP_PERSIST_KB_PER_WORLD": "1"}, 1024, 0),
], ids=["scratch", "scratch_fixed_region", "persistent", "both"])
def test_constructor_overflow_reruns(built, monkeypatch, env, num_worlds, flags):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _lock_step(num_worlds, 11, flags, (1, 7, 40))


def test_jittered_fans_at_8192_worlds(built):
    # about 10.7 KB of constructor scratch per world: more than the default
    # 64 MiB scratch region at 8192 worlds
    _lock_step(8192, 5, 2, (1, 7))
