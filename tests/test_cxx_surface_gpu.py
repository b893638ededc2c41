"""GPU: the C++ classes of <madrona/mw_gpu.hpp> that wrap the executor objects,
RUN once each.  Every tests/shims/*_conformance.inl defines `<prefix>_cycle`,
which calls every member of its class on a caller's executor and returns a
value its comment documents (0: a tensor's dims or pointers were not as they
should be); the *_abi.py tests only see that it links.  Here it is called on a
live simulator's own MWCudaExecutor (sim_hip_cxx_exec), for the host and the
gfx950 translation unit of each kind, on the smallest shapes at which a
wrapper's dims can be wrong: 3 worlds, two columns, max_rows 2, two reduce
terms of different result types, 5 handles, 3 x 2 rays, 3 x 2 boxes of 4 hits.
Afterwards the simulator still synchronizes and steps, and its step launches
are what they were: _cycle sets a step object and unsets it again.

The wrappers abort() on any non-zero code of the runtime."""
import ctypes as C
import os

import numpy as np
import pytest

from madrona_amd import reduce_ref, simlib
from madrona_amd.simlib import HIP_BUILD_DIR, Simulator, hip_lib_path

pytestmark = pytest.mark.gpu

WORLDS = 3
PREFIXES = ("host", "hip")


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _launches(sim):
    return [k["name"] for k in sim.profile(1)]


def _open(make):
    with make() as sim:
        exec_ = sim.lib.sim_hip_cxx_exec(sim.handle)
        assert exec_, "sim_hip_cxx_exec gave no executor"
        yield sim, exec_, _launches(sim)


@pytest.fixture(scope="module")
def stress(built):
    yield from _open(lambda: Simulator(hip_lib_path("sort_stress"), WORLDS, seed=7))


@pytest.fixture(scope="module")
def broadphase(built):
    yield from _open(lambda: Simulator(hip_lib_path("broadphase_only"), WORLDS, seed=3, flags=1))


def _cycle(library, prefix, restype, *argtypes):
    simlib.runtime_lib()    # (libmadrona_hip.so, RTLD_GLOBAL: the shim links against it)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, f"lib{library}_conformance.so"))
    fn = getattr(lib, prefix + "_cycle")
    fn.restype = restype
    fn.argtypes = [C.c_void_p, *argtypes]
    return fn


def _ids(sim, column):
    """(archetype id, component id, cell bytes) of a dump-list column"""
    idx = [c[0] for c in sim.columns].index(column)
    arch, comp = C.c_uint32(0), C.c_uint32(0)
    assert sim.lib.sim_hip_column_ids(sim.handle, idx, C.byref(arch), C.byref(comp)) == 0
    return arch.value, comp.value, sim.columns[idx][1]


def _table(sim, columns):
    """(the one archetype id, the component ids as a C array, the first cell's bytes)"""
    ids = [_ids(sim, c) for c in columns]
    assert len({a for a, _, _ in ids}) == 1
    return ids[0][0], (C.c_uint32 * len(ids))(*[c for _, c, _ in ids]), ids[0][2]


def _still_runs_with_nothing_set(sim, launches):
    sim.sync()
    sim.step()
    assert _launches(sim) == launches


@pytest.mark.parametrize("prefix", PREFIXES)
def test_snapshot(stress, prefix):
    sim, exec_, launches = stress
    with sim.snapshot() as snap:
        snap.save()
        want = snap.nbytes
    assert want > 0
    got = _cycle("snapshot", f"snapconf_{prefix}", C.c_uint64)(exec_)
    assert got == want      # (the bytes a save of the same state holds)
    _still_runs_with_nothing_set(sim, launches)


@pytest.mark.parametrize("prefix", PREFIXES)
def test_digest(stress, prefix):
    sim, exec_, launches = stress
    ids = [_ids(sim, c) for c in ("Item.Key", "Item.Vec3", "Scratch.Vec3")]
    plan = (simlib.DigestColumn * 3)(*[simlib.DigestColumn(a, c) for a, c, _ in ids])
    got = _cycle("digest", f"digconf_{prefix}", C.c_uint32,
                 C.POINTER(simlib.DigestColumn), C.c_uint32)(exec_, plan, 3)
    assert got == len({a for a, _, _ in ids}) == 2      # (a group per table listed)
    _still_runs_with_nothing_set(sim, launches)


@pytest.mark.parametrize("prefix", PREFIXES)
@pytest.mark.parametrize("library,stem", [("view", "viewconf"), ("world_write", "writeconf")])
def test_view_and_write(stress, library, stem, prefix):
    sim, exec_, launches = stress
    max_rows = 2
    arch, comps, cell = _table(sim, ["Item.Vec3", "Item.Key"])
    got = _cycle(library, f"{stem}_{prefix}", C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                 C.c_uint32, C.c_uint32)(exec_, arch, comps, 2, max_rows)
    assert got == cell * max_rows == 24     # (the first column's cell bytes x max_rows)
    _still_runs_with_nothing_set(sim, launches)


@pytest.mark.parametrize("prefix", PREFIXES)
def test_reduce(stress, prefix):
    """One term of each result type: Float32 (F32 SUM) and Int32 (U32
    COUNT_NONZERO); _cycle checks every term's tensor type and elems."""
    sim, exec_, launches = stress
    arch, comps, cell = _table(sim, ["Item.Vec3", "Item.Key"])
    terms = (simlib.ReduceTerm * 2)(
        simlib.ReduceTerm(comps[0], 0, cell // 4, reduce_ref.DTYPES["f32"],
                          reduce_ref.OPS["sum"], 0, 0.0),
        simlib.ReduceTerm(comps[1], 0, 1, reduce_ref.DTYPES["u32"],
                          reduce_ref.OPS["count_nonzero"], 0, 0.0))
    got = _cycle("reduce", f"reduceconf_{prefix}", C.c_uint32, C.c_uint32,
                 C.POINTER(simlib.ReduceTerm), C.c_uint32)(exec_, arch, terms, 2)
    assert got == terms[0].num_elems == 3       # (the first term's elems)
    _still_runs_with_nothing_set(sim, launches)


@pytest.mark.parametrize("prefix", PREFIXES)
@pytest.mark.parametrize("library", ["gather", "scatter"])
def test_gather_and_scatter(stress, library, prefix):
    """(the scatter's select is zero at creation: nothing is stored)"""
    sim, exec_, launches = stress
    torch = _torch()
    handles = torch.zeros((5, 2), dtype=torch.int32, device=torch.device("cuda", sim.gpu_id))
    torch.cuda.synchronize()
    _, comp, cell = _ids(sim, "Item.Vec3")
    source = simlib.GatherSource(handles.data_ptr(), 5, 8, 0, 1, 0)
    comps = (C.c_uint32 * 1)(comp)
    got = _cycle(library, f"{library}conf_{prefix}", C.c_uint64, C.POINTER(simlib.GatherSource),
                 C.POINTER(C.c_uint32), C.c_uint32)(exec_, C.byref(source), comps, 1)
    assert got == cell * 5 == 60        # (the component's cell bytes x handles)
    _still_runs_with_nothing_set(sim, launches)
    del handles


@pytest.mark.parametrize("prefix", PREFIXES)
def test_rings(stress, prefix):
    sim, exec_, launches = stress
    torch = _torch()
    _, dtype, dims, _ = sim.tensor_meta("churn")
    slot_bytes = int(np.prod(dims)) * dtype.itemsize
    rings = torch.zeros((2, 2, slot_bytes), dtype=torch.uint8,
                        device=torch.device("cuda", sim.gpu_id))
    torch.cuda.synchronize()
    ptr = sim.tensor_ptr("churn")
    got = _cycle("ring", f"ringconf_{prefix}", C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                 C.c_void_p, C.c_uint64, C.c_uint32)(
        exec_, ptr, rings[0].data_ptr(), ptr, rings[1].data_ptr(), slot_bytes, 2)
    assert got == 0     # (no replay ran between setting the rings and asking)
    _still_runs_with_nothing_set(sim, launches)
    del rings


@pytest.mark.parametrize("prefix", PREFIXES)
def test_rays(broadphase, prefix):
    sim, exec_, launches = broadphase
    fans, per_fan = 3, 2
    desc = simlib.RaysDesc(fans, per_fan, 0, 0)     # (world and origin are owned)
    got = _cycle("rays", f"raysconf_{prefix}", C.c_uint64,
                 C.POINTER(simlib.RaysDesc))(exec_, C.byref(desc))
    assert got == (fans * per_fan) * fans == 18     # (rays x fans)
    _still_runs_with_nothing_set(sim, launches)


@pytest.mark.parametrize("prefix", PREFIXES)
def test_boxes(broadphase, prefix):
    sim, exec_, launches = broadphase
    bundles, per_bundle, max_hits = 3, 2, 4
    desc = simlib.BoxesDesc(bundles, per_bundle, max_hits, 0, 0, 0)    # (world, centre owned)
    got = _cycle("boxes", f"boxesconf_{prefix}", C.c_uint64,
                 C.POINTER(simlib.BoxesDesc))(exec_, C.byref(desc))
    assert got == (bundles * per_bundle) * max_hits * bundles == 72     # (boxes x hits x bundles)
    _still_runs_with_nothing_set(sim, launches)
