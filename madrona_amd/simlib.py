"""ctypes binding for the simulator C API in sims/common/sim_c_api.h.

The same wrapper drives a simulator built against the MI355X HIP backend
(``lib<sim>_hip.so``) and one built against the reference CPU backend
(``oracle/_ref/lib<sim>_ref.so``); only tests/, ``__graft_entry__.smoke`` and
bench.py's ``cpu_baseline`` leg are allowed to load the latter.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Tuple

import numpy as np

from . import digest_ref

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_BUILD_DIR = os.path.join(REPO_ROOT, "madrona_amd",
                             os.environ.get("MADRONA_HIP_BUILD_DIR", "_build"))
REF_BUILD_DIR = os.path.join(REPO_ROOT, "oracle", "_ref")

SIM_DTYPES = {
    0: np.uint8, 1: np.int8, 2: np.int16, 3: np.int32, 4: np.int64,
    5: np.float16, 6: np.float32,
}


class SimCreateArgs(C.Structure):
    _fields_ = [
        ("num_worlds", C.c_uint32),
        ("seed", C.c_uint32),
        ("gpu_id", C.c_int32),
        ("num_workers", C.c_uint32),
        ("world_base", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class SimTensorInfo(C.Structure):
    _fields_ = [
        ("name", C.c_char_p),
        ("dtype", C.c_int32),
        ("ndim", C.c_int32),
        ("dims", C.c_int64 * 4),
        ("on_device", C.c_int32),
    ]


class SimColumnInfo(C.Structure):
    _fields_ = [
        ("name", C.c_char_p),
        ("elem_bytes", C.c_uint32),
        ("is_float", C.c_int32),
    ]


def hip_lib_path(sim: str) -> str:
    return os.path.join(HIP_BUILD_DIR, f"lib{sim}_hip.so")


def ref_lib_path(sim: str, speed: bool = False) -> str:
    suffix = "_ref_speed.so" if speed else "_ref.so"
    return os.path.join(REF_BUILD_DIR, f"lib{sim}{suffix}")


def _bind(lib: C.CDLL) -> None:
    lib.sim_create.restype = C.c_void_p
    lib.sim_create.argtypes = [C.POINTER(SimCreateArgs)]
    lib.sim_destroy.argtypes = [C.c_void_p]
    lib.sim_backend.restype = C.c_char_p
    lib.sim_backend.argtypes = [C.c_void_p]
    lib.sim_step.argtypes = [C.c_void_p, C.c_uint32]
    lib.sim_num_tensors.restype = C.c_uint32
    lib.sim_num_tensors.argtypes = [C.c_void_p]
    lib.sim_tensor_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(SimTensorInfo)]
    lib.sim_tensor_ptr.restype = C.c_void_p
    lib.sim_tensor_ptr.argtypes = [C.c_void_p, C.c_uint32]
    lib.sim_tensor_read.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    lib.sim_tensor_write.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    lib.sim_num_columns.restype = C.c_uint32
    lib.sim_num_columns.argtypes = [C.c_void_p]
    lib.sim_column_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(SimColumnInfo)]
    lib.sim_column_dump.restype = C.c_int64
    lib.sim_column_dump.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                    C.POINTER(C.c_int32)]
    lib.sim_hip_run_taskgraph.restype = C.c_int
    lib.sim_hip_run_taskgraph.argtypes = [C.c_void_p, C.c_uint32]
    lib.sim_column_dump_raw.restype = C.c_int64
    lib.sim_column_dump_raw.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    lib.sim_hip_exec.restype = C.c_void_p
    lib.sim_hip_exec.argtypes = [C.c_void_p]
    lib.sim_hip_render.restype = C.c_int
    lib.sim_hip_render.argtypes = [C.c_void_p]
    lib.sim_hip_render_graph.restype = C.c_uint64
    lib.sim_hip_render_graph.argtypes = [C.c_void_p]
    lib.sim_hip_step_graph.restype = C.c_uint64
    lib.sim_hip_step_graph.argtypes = [C.c_void_p]
    # (a simulator library built before the accessor was added does not have it:
    # a reference-backend library an earlier build left behind still loads)
    if hasattr(lib, "sim_hip_cxx_exec"):
        lib.sim_hip_cxx_exec.restype = C.c_void_p
        lib.sim_hip_cxx_exec.argtypes = [C.c_void_p]
    # (a simulator library built before state digests does not have it)
    if hasattr(lib, "sim_hip_column_ids"):
        lib.sim_hip_column_ids.restype = C.c_int
        lib.sim_hip_column_ids.argtypes = [C.c_void_p, C.c_uint32,
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]


class KernelStat(C.Structure):
    _fields_ = [
        ("name", C.c_char_p),
        ("node_kind", C.c_uint32),
        ("archetype_id", C.c_uint32),
        ("avg_us", C.c_double),
        ("algo_bytes", C.c_double),
        ("rows", C.c_double),
        ("io_declared", C.c_uint32),
        ("workgroups", C.c_uint32),
        ("node_index", C.c_uint32),
        ("pad_", C.c_uint32),
    ]


class DigestColumn(C.Structure):
    """mwhip_digest_column (include/mwhip.h)"""
    _fields_ = [("archetype_id", C.c_uint32), ("component_id", C.c_uint32)]


class ReduceTerm(C.Structure):
    """mwhip_reduce_term (include/mwhip.h)"""
    _fields_ = [("component_id", C.c_uint32), ("byte_offset", C.c_uint32),
                ("num_elems", C.c_uint32), ("dtype", C.c_uint32), ("op", C.c_uint32),
                ("flags", C.c_uint32), ("limit", C.c_float)]


class GatherSource(C.Structure):
    """mwhip_gather_source (include/mwhip.h)."""
    _fields_ = [("src", C.c_void_p), ("num_records", C.c_uint64),
                ("record_bytes", C.c_uint32), ("first_byte", C.c_uint32),
                ("handles_per_record", C.c_uint32), ("pad_", C.c_uint32)]


class RaySource(C.Structure):
    """mwhip_ray_source (include/mwhip.h)."""
    _fields_ = [("src", C.c_void_p), ("record_bytes", C.c_uint32), ("first_byte", C.c_uint32)]


class RaysDesc(C.Structure):
    """mwhip_rays_desc (include/mwhip.h)."""
    _fields_ = [("num_fans", C.c_uint32), ("rays_per_fan", C.c_uint32),
                ("fans_per_world", C.c_uint32), ("pad_", C.c_uint32),
                ("world", RaySource), ("count", RaySource), ("origin", RaySource)]


class BoxesDesc(C.Structure):
    """mwhip_boxes_desc (include/mwhip.h)."""
    _fields_ = [("num_bundles", C.c_uint32), ("boxes_per_bundle", C.c_uint32),
                ("max_hits", C.c_uint32), ("bundles_per_world", C.c_uint32),
                ("flags", C.c_uint32), ("pad_", C.c_uint32),
                ("world", RaySource), ("count", RaySource), ("centre", RaySource)]


class ContactsDesc(C.Structure):
    """mwhip_contacts_desc (include/mwhip.h)."""
    _fields_ = [("max_contacts", C.c_uint32), ("flags", C.c_uint32),
                ("own_select", C.c_uint32), ("pad_", C.c_uint32), ("select", RaySource)]


class ShapesDesc(C.Structure):
    """mwhip_shapes_desc (include/mwhip.h)."""
    _fields_ = [("num_bundles", C.c_uint32), ("shapes_per_bundle", C.c_uint32),
                ("max_hits", C.c_uint32), ("num_objects", C.c_uint32),
                ("bundles_per_world", C.c_uint32), ("flags", C.c_uint32),
                ("world", RaySource), ("count", RaySource), ("exclude", RaySource)]


class SortStats(C.Structure):
    """mwhip_sort_counters (include/mwhip.h)"""
    _fields_ = [(name, C.c_uint64) for name in
                ("runs", "stay_runs", "rows_copied", "rows_in", "rows_out", "tail_rows")]


class SortReuseStats(C.Structure):
    """mwhip_sort_reuse_counters (include/mwhip.h)"""
    _fields_ = [("skipped_runs", C.c_uint64), ("rows_reused", C.c_uint64)]


def _torch_runtime_first() -> None:
    """PyTorch-ROCm bundles its own HIP / HSA runtime; a process that loads the
    system runtime first (through our libraries) and torch afterwards ends up
    with two HSA runtimes and torch reports "No HIP GPUs are available".
    Loading torch's copy first makes our libraries bind to it (same SONAME)."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


_U32P, _U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_OBJECT = [C.c_void_p, C.c_uint64]      # (the executor, the object's handle)

# The executor objects of include/mwhip.h by the stem of their calls: the verbs
# (mwhip_<stem>_<verb> and ..._<verb>_async) and the getters of further
# per-object device pointers (mwhip_<stem>_<getter>).  Each has
# mwhip_<stem>_destroy, and each but the snapshot mwhip_set_step_<stem>.
_KINDS = {
    "snapshot": (("save", "restore"), ()),
    "digest": (("compute",), ()),
    "view": (("compute",), ("counts",)),
    "write": (("apply",), ("take", "counts")),
    "reduce": (("compute",), ("counts", "alarm")),
    "gather": (("compute",), ("archetypes", "worlds")),
    "scatter": (("apply",), ("select", "archetypes", "worlds", "written")),
    "rays": (("compute",), ()),
    "boxes": (("compute",), ()),
    "contacts": (("compute",), ()),
    "shapes": (("compute",), ()),
}

_runtime = None


def _declare(lib: C.CDLL, name: str, restype, argtypes) -> None:
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = argtypes


def runtime_lib() -> C.CDLL:
    """libmadrona_hip.so (the C ABI of include/mwhip.h), opened and declared
    by the first call."""
    global _runtime
    if _runtime is not None:
        return _runtime
    _torch_runtime_first()
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    lib.mwhip_profile.restype = C.c_int32
    lib.mwhip_profile.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32,
                                  C.POINTER(KernelStat), C.c_uint32]
    lib.mwhip_last_error.restype = C.c_char_p
    lib.mwhip_stream.restype = C.c_void_p
    lib.mwhip_stream.argtypes = [C.c_void_p]
    lib.mwhip_run_async.restype = C.c_int
    lib.mwhip_run_async.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.mwhip_synchronize.restype = C.c_int
    lib.mwhip_synchronize.argtypes = [C.c_void_p]
    lib.mwhip_build_launch_graph_with_pack.restype = C.c_int
    lib.mwhip_build_launch_graph_with_pack.argtypes = [
        C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p),
        C.POINTER(C.c_uint32), C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.mwhip_stream_wait_replays.restype = C.c_int
    lib.mwhip_stream_wait_replays.argtypes = [C.c_void_p, C.c_void_p]
    lib.mwhip_set_input_ring.restype = C.c_int
    lib.mwhip_set_input_ring.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_uint64, C.c_uint32]
    lib.mwhip_set_output_ring.restype = C.c_int
    lib.mwhip_set_output_ring.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_uint64, C.c_uint32, C.c_uint32]
    lib.mwhip_output_ring_recorded.restype = C.c_int
    lib.mwhip_output_ring_recorded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32,
                                               C.POINTER(C.c_uint64)]
    lib.mwhip_mark_window.restype = C.c_int
    lib.mwhip_mark_window.argtypes = [C.c_void_p, C.c_uint32]
    lib.mwhip_pack_rows.restype = C.c_int
    lib.mwhip_pack_rows.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_uint32), C.c_uint32, C.c_void_p]
    # what every kind has ...
    for stem, (verbs, getters) in _KINDS.items():
        _declare(lib, f"mwhip_{stem}_destroy", None, _OBJECT)
        for verb in verbs:
            _declare(lib, f"mwhip_{stem}_{verb}", C.c_int, _OBJECT)
            _declare(lib, f"mwhip_{stem}_{verb}_async", C.c_int, _OBJECT)
        for getter in getters:
            _declare(lib, f"mwhip_{stem}_{getter}", C.c_void_p, _OBJECT)
        if stem != "snapshot":
            # (the executor has one step digest: set by its handle, unset by 0)
            _declare(lib, f"mwhip_set_step_{stem}", C.c_int,
                     _OBJECT if stem == "digest" else _OBJECT + [C.c_int])
    # ... and what is a kind's own: how it is made and how its buffers are asked for
    _declare(lib, "mwhip_snapshot_create", C.c_int, [C.c_void_p, _U64P])
    _declare(lib, "mwhip_snapshot_bytes", C.c_uint64, _OBJECT)
    _declare(lib, "mwhip_digest_create", C.c_int,
             [C.c_void_p, C.POINTER(DigestColumn), C.c_uint32, _U64P])
    _declare(lib, "mwhip_digest_buffer", C.c_void_p, _OBJECT + [_U32P, _U32P])
    _declare(lib, "mwhip_digest_group", C.c_int, _OBJECT + [C.c_uint32, _U32P, _U32P])
    for stem in ("view", "write"):
        _declare(lib, f"mwhip_{stem}_create", C.c_int,
                 [C.c_void_p, C.c_uint32, _U32P, C.c_uint32, C.c_uint32, _U64P])
    _declare(lib, "mwhip_reduce_create", C.c_int,
             [C.c_void_p, C.c_uint32, C.POINTER(ReduceTerm), C.c_uint32, _U64P])
    for stem in ("gather", "scatter"):
        _declare(lib, f"mwhip_{stem}_create", C.c_int,
                 [C.c_void_p, C.POINTER(GatherSource), _U32P, C.c_uint32, _U64P])
    for stem in ("view", "write", "reduce", "gather", "scatter"):
        _declare(lib, f"mwhip_{stem}_buffer", C.c_void_p, _OBJECT + [C.c_uint32, _U64P, _U32P])
    for stem, desc in (("rays", RaysDesc), ("boxes", BoxesDesc), ("contacts", ContactsDesc),
                       ("shapes", ShapesDesc)):
        _declare(lib, f"mwhip_{stem}_create", C.c_int, [C.c_void_p, C.POINTER(desc), _U64P])
        _declare(lib, f"mwhip_{stem}_buffer", C.c_void_p, _OBJECT + [C.c_uint32, _U64P])
    _declare(lib, "mwhip_set_ray_kernel", C.c_int, [C.c_void_p, C.c_void_p])
    _declare(lib, "mwhip_set_box_kernel", C.c_int, [C.c_void_p, C.c_void_p])
    _declare(lib, "mwhip_set_contact_kernel", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32])
    _declare(lib, "mwhip_set_shape_kernel", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32])
    _runtime = lib
    return lib


def _verb(verb: str, returns_self: bool, doc: str = None):
    """Method `verb` of an _ExecObject: mwhip_<stem>_<verb>(executor, handle),
    checked.  (One frame per call: this is the path of a per-step call.)"""
    def call(self):
        handle = self._live()
        fn, name = self._calls[verb]
        self._check(fn(self._exec, handle), name)
        return self if returns_self else None
    call.__name__ = call.__qualname__ = verb
    call.__doc__ = doc
    return call


class _Checked:
    """A wrapper of executor calls that is closed like a file: _check() raises
    with the runtime's message, `with` closes."""

    _rt = None

    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            raise RuntimeError(f"{what} -> {rc}: {self._rt.mwhip_last_error().decode()}")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _ExecObject(_Checked):
    """What Snapshot, StateDigest, WorldView, WorldWrite, WorldReduce, EntityGather, EntityScatter, RayQuery, BoxQuery, ContactQuery and ShapeQuery are: something a simulator's
    executor owns, named by `handle` there, kept in one of the simulator's
    lists (`_list`) while it is open.  close() frees it and takes it off the
    list (a snapshot too, which used to stay on it until the simulator closed); Simulator.close() frees the executor and orphans
    what is left: close() then does nothing, anything else raises.

    A kind names its calls by `_stem` (a key of _KINDS) and says in __init__
    what is its own: _open(sim), _create(what mwhip_<stem>_create takes between
    the executor and the handle), then its buffers.  The rest is here: the
    calls by their verb (_verb), the torch tensors over device buffers (_wrap,
    _int32), which are made once and dropped with the object."""

    _kind = "object"    # in messages
    _stem = ""          # mwhip_<stem>_*
    _list = ""          # the simulator's list of the open ones
    _lists: List[str] = []      # (every kind's, as the classes are defined)
    _sim = None
    _exec = 0
    _calls: Dict[str, tuple] = {}
    handle = 0

    def __init_subclass__(cls):
        if "_list" in vars(cls):
            _ExecObject._lists.append(cls._list)

    def _open(self, sim: "Simulator") -> None:
        self._sim = sim
        self._rt = runtime_lib()
        self._exec = sim.hip_exec()
        self._tensors = {}
        self._every_step = False
        self.handle = 0
        # (the runtime's functions are looked up here, once, not by every call)
        names = {verb + tail: f"mwhip_{self._stem}_{verb}{tail}"
                 for verb in _KINDS[self._stem][0] for tail in ("", "_async")}
        if self._stem != "snapshot":
            names["set_step"] = f"mwhip_set_step_{self._stem}"
        self._calls = {verb: (getattr(self._rt, name), name) for verb, name in names.items()}

    def _create(self, *args) -> None:
        handle = C.c_uint64(0)
        name = f"mwhip_{self._stem}_create"
        self._check(getattr(self._rt, name)(self._exec, *args, C.byref(handle)), name)
        self.handle = int(handle.value)

    def _live(self) -> int:
        # (the executor pointer dies with the simulator: never passed on then)
        if self._sim is None:
            raise RuntimeError(f"this {self._kind} is closed (or its simulator is)")
        return self.handle

    def _pointer(self, getter: str) -> int:
        """mwhip_<stem>_<getter>: a further device buffer of the object"""
        return int(getattr(self._rt, f"mwhip_{self._stem}_{getter}")(
            self._exec, self.handle) or 0)

    def _wrap(self, key, ptr, dtype, shape):
        if key not in self._tensors:
            import torch

            from .tensor import DeviceColumn
            self._tensors[key] = torch.as_tensor(
                DeviceColumn(ptr, dtype, shape),
                device=torch.device("cuda", self._sim.gpu_id))
        return self._tensors[key]

    def _int32(self, name: str, ptr: int, n: int):
        """torch int32 [n] over a device buffer (no copy)"""
        self._live()
        return self._wrap(("", name), ptr, np.int32, (n,))

    def _orphan(self) -> None:
        """Simulator.close(): the executor has freed (or is about to free) it."""
        self.handle = 0
        self._exec = 0
        self._sim = None
        self._tensors = {}

    def close(self) -> None:
        if self._sim is not None:
            if self.handle:
                getattr(self._rt, f"mwhip_{self._stem}_destroy")(self._exec, self.handle)
            open_ones = getattr(self._sim, self._list)
            if self in open_ones:
                open_ones.remove(self)
        self._orphan()


class _StepObject(_ExecObject):
    """An executor object that a step graph can carry: every_step()."""

    def _step_args(self, handle: int, on: bool) -> tuple:
        return handle, 1 if on else 0

    def every_step(self, on: bool = True) -> None:
        """Every replay of a step graph computes or applies this object (waits
        for the stream and rebuilds the launch graphs); on=False turns it off
        again."""
        handle = self._live()
        if not on and not self._every_step:
            return
        fn, name = self._calls["set_step"]
        self._check(fn(self._exec, *self._step_args(handle, on)), name)
        self._every_step = bool(on)
        # (the rebuilt graphs are looked up by the same handles)


class _Computed:
    """The verbs of a _StepObject that is computed."""

    compute = _verb("compute", True,
                    "Rewrites every output in full; waits for the executor's stream.")
    compute_async = _verb("compute_async", False)


class _Applied:
    """The verbs of a _StepObject that is applied."""

    apply = _verb("apply", True, "Writes into the tables; waits for the executor's stream.")
    apply_async = _verb("apply_async", False)


class _Cells(_StepObject):
    """A _StepObject with a device buffer of uint8 [*_shape(), cell_bytes] per
    listed name (a column or a component): mwhip_<stem>_buffer."""

    def _shape(self) -> tuple:
        raise NotImplementedError

    def _open_buffers(self, names) -> None:
        buffer = getattr(self._rt, f"mwhip_{self._stem}_buffer")
        self._buffers = {}
        for p, name in enumerate(names):
            nbytes, cell = C.c_uint64(0), C.c_uint32(0)
            ptr = buffer(self._exec, self.handle, p, C.byref(nbytes), C.byref(cell))
            assert ptr and nbytes.value == int(np.prod(self._shape())) * cell.value
            self._buffers[name] = (int(ptr), int(cell.value))

    def buffer_ptr(self, name: str) -> int:
        """Device address of the [*shape, cell_bytes] bytes of `name`."""
        self._live()
        return self._buffers[name][0]

    def cell_bytes(self, name: str) -> int:
        return self._buffers[name][1]

    def tensor(self, name: str, dtype=None):
        """torch uint8 [*shape, cell_bytes] over the device buffer of `name` (no
        copy), or, with a numpy dtype, [*shape, cell_bytes // itemsize] of that
        type.  shape: worlds, max_rows of a view or a write; N of a gather or a
        scatter."""
        self._live()
        ptr, cell = self._buffers[name]
        dt = np.dtype(np.uint8 if dtype is None else dtype)
        if cell % dt.itemsize != 0:
            raise TypeError(f"{name}: cells of {cell} bytes do not hold whole {dt} items")
        return self._wrap((name, dt.str), ptr, dt.type, (*self._shape(), cell // dt.itemsize))


def _need_column_ids(sim: "Simulator") -> None:
    if not hasattr(sim.lib, "sim_hip_column_ids"):
        raise RuntimeError("this simulator library has no sim_hip_column_ids: rebuild it")


def _column_ids(sim: "Simulator", idx: int, label=None) -> Tuple[int, int]:
    """(archetype id, component id) of dump-list column idx; label: how a
    message names the column"""
    arch, comp = C.c_uint32(0), C.c_uint32(0)
    if sim.lib.sim_hip_column_ids(sim.handle, idx, C.byref(arch), C.byref(comp)) != 0:
        raise RuntimeError(f"sim_hip_column_ids({idx if label is None else label}) failed")
    return int(arch.value), int(comp.value)


def _table_columns(sim: "Simulator", table: str, who: str):
    """(every dump-list column's name, those of `table`)"""
    names = [c[0] for c in sim._columns]
    of_table = [n for n in names if n.split(".", 1)[0] == table]
    if not of_table:
        raise KeyError(f"{who}: no table {table!r} in the dump list")
    return names, of_table


def _one_table(sim: "Simulator", names, columns) -> Tuple[int, List[int]]:
    """(the archetype id, the component ids) of columns of one table"""
    ids = [_column_ids(sim, names.index(name), name) for name in columns]
    archetypes = {arch for arch, _ in ids}
    assert len(archetypes) == 1, archetypes
    return archetypes.pop(), [comp for _, comp in ids]


class Snapshot(_ExecObject):
    """One saved copy of all world state of a HIP-backend simulator, in device
    memory (mwhip_snapshot_*, include/mwhip.h): save() / restore() wait,
    save_async() / restore_async() are queued on the executor's stream behind
    the replays queued so far (step_async).  Reusable; belongs to the
    simulator that made it; Simulator.close() frees what is left and empties
    those snapshots (their close() then does nothing, any other call raises).
    Not rewound: the executor's replay count (the input
    ring's slot position) and the rgb / depth outputs of the render pass."""

    _kind, _stem, _list = "snapshot", "snapshot", "_snapshots"

    def __init__(self, sim: "Simulator"):
        self._open(sim)
        if not self._exec:
            raise RuntimeError("snapshots need the HIP backend")
        self._create()

    save, restore = _verb("save", False), _verb("restore", False)
    save_async, restore_async = _verb("save_async", False), _verb("restore_async", False)

    @property
    def nbytes(self) -> int:
        """Bytes the last save holds (waits for the executor's stream)."""
        return int(self._rt.mwhip_snapshot_bytes(self._exec, self._live()))


RING_ON_STEP = 0      # MWHIP_RING_ON_STEP
RING_ON_RENDER = 1    # MWHIP_RING_ON_RENDER


class Trajectory(_Checked):
    """Exported tensors of a HIP-backend simulator recorded per step on the
    device (mwhip_set_output_ring, include/mwhip.h): traj[name] is a torch
    tensor [steps, *dims] of the tensor's dtype on the simulator's device, and
    the k-th replay after record() -- of the step graph, or of the render graph
    with on_render -- leaves the tensor as it is when the replay ends in slot
    k % steps.  Nothing foreign sits on the executor's stream between two
    replays: queue them with step_async and read when they are done (sync(),
    stream_wait_replays()); a slot that a replay still queued will rewrite must
    not be read before that replay is through.  A ring is named by (tensor,
    kind) on the executor, so a tensor that an open trajectory of the same kind
    already records is refused (ValueError) rather than taken over.  close()
    removes the rings and lets the simulator forget the trajectory;
    Simulator.close() orphans what is left (the tensors stay valid)."""

    _list = "_trajectories"     # the simulator's list of the open ones

    def __init__(self, sim: "Simulator", names: List[str], steps: int,
                 on_render: bool = False):
        import torch

        self._rt = runtime_lib()
        self._exec = sim.hip_exec()
        if not self._exec:
            raise RuntimeError("recording needs the HIP backend")
        if steps < 1:
            raise ValueError("record(): at least one step")
        self.steps = int(steps)
        self._when = RING_ON_RENDER if on_render else RING_ON_STEP
        names = list(names)
        taken = [name for name in names if names.count(name) > 1 or any(
            other._when == self._when and name in other._srcs
            for other in sim._trajectories)]
        if taken:
            raise ValueError(
                f"record(): {sorted(set(taken))} named twice or already recorded by an "
                "open trajectory of this kind (close() it first)")
        # (the simulator's list of open trajectories; close() leaves it)
        self._open_in = sim._trajectories
        self._tensors: Dict[str, "torch.Tensor"] = {}
        self._srcs: Dict[str, int] = {}
        device = torch.device("cuda", sim.gpu_id)
        for name in names:
            _, dtype, dims, _ = sim.tensor_meta(name)
            self._tensors[name] = torch.zeros(
                (self.steps, *dims), device=device,
                dtype=torch.from_numpy(np.empty(0, dtype)).dtype)
        # (the fills run on torch's stream, the replays on the executor's)
        torch.cuda.synchronize(device)
        try:
            for name, ring in self._tensors.items():
                src = sim.tensor_ptr(name)
                self._check(self._rt.mwhip_set_output_ring(
                    self._exec, src, ring.data_ptr(),
                    ring[0].numel() * ring.element_size(), self.steps, self._when),
                    f"mwhip_set_output_ring({name})")
                self._srcs[name] = src
        except Exception:
            self.close()
            raise

    def _orphan(self) -> None:
        """Simulator.close(): the executor (and its rings) is gone."""
        self._exec = 0
        self._srcs = {}
        self._open_in = None

    def __getitem__(self, name: str):
        return self._tensors[name]

    @property
    def names(self) -> List[str]:
        return list(self._tensors.keys())

    @property
    def recorded(self) -> int:
        """Replays that have recorded since record() (waits for the executor's
        stream; not taken modulo `steps`)."""
        if not self._exec or not self._srcs:
            raise RuntimeError("this trajectory is closed (or its simulator is)")
        out = C.c_uint64(0)
        self._check(self._rt.mwhip_output_ring_recorded(
            self._exec, next(iter(self._srcs.values())), self._when, C.byref(out)),
            "mwhip_output_ring_recorded")
        return int(out.value)

    def slot(self, k: int) -> int:
        """Index along dimension 0 of what replay k (0-based) recorded."""
        return int(k) % self.steps

    def close(self) -> None:
        """Removes the rings (waits for the executor's stream); the tensors keep
        what has been recorded."""
        if self._exec:
            for name, src in self._srcs.items():
                self._rt.mwhip_set_output_ring(self._exec, src, None, 0, 0, self._when)
        self._srcs = {}
        self._exec = 0
        # the simulator keeps open trajectories only: the ring tensors live as
        # long as the caller holds this object, no longer
        if self._open_in is not None:
            if self in self._open_in:
                self._open_in.remove(self)
            self._open_in = None


class StateDigest(_Computed, _StepObject):
    """A 64-bit hash per world of a list of dump-list columns, one row of
    hashes per table the list names (madrona_amd/digest_ref.py is the exact
    definition; mwhip_digest_*, include/mwhip.h, computes it on the device).
    compute() returns a numpy uint64 [groups, worlds] on either backend, and the
    same call gives the same numbers on both: on the HIP backend one kernel
    hashes the tables where they are (sorted or not), on the reference backend
    digest_ref is evaluated over dump_all().  It is a hash of the multiset of a
    world's rows in each table: blind to the order of a world's rows.  Columns
    that hold pointers differ between executors: list value columns only.
    HIP backend only: compute_async() queues the computation on the executor's
    stream behind the replays queued so far, `tensor` is a zero-copy torch int64
    view [groups, worlds] of the device buffer, every_step() makes every replay
    of a step graph recompute the digest (before its output rings: a ring over
    `buffer_ptr` records the digest of every step).  close() frees it;
    Simulator.close() orphans what is left."""

    _kind, _stem, _list = "digest", "digest", "_digests"

    def __init__(self, sim: "Simulator", columns=None):
        names = [c[0] for c in sim._columns]
        if columns is None:
            columns = list(range(len(names)))
        self._indices: List[int] = []
        for col in columns:
            idx = names.index(col) if isinstance(col, str) else int(col)
            if not 0 <= idx < len(names):
                raise IndexError(f"digest(): no dump-list column {col!r}")
            self._indices.append(idx)
        if not self._indices:
            raise ValueError("digest(): no columns")
        if len(set(self._indices)) != len(self._indices):
            raise ValueError("digest(): a column is listed twice")
        self._tables = [names[i].split(".", 1)[0] for i in self._indices]
        self.num_worlds = sim.num_worlds
        if sim.backend != "hip":
            # (no executor and no runtime: _rt stays None)
            self._sim = sim
            self.groups = [key for key, _, _ in digest_ref.plan_groups(self._tables)]
            return
        _need_column_ids(sim)
        self._open(sim)
        plan = (DigestColumn * len(self._indices))(
            *[DigestColumn(*_column_ids(sim, idx)) for idx in self._indices])
        self._create(plan, len(self._indices))
        num_groups, num_worlds = C.c_uint32(0), C.c_uint32(0)
        self.buffer_ptr = int(self._rt.mwhip_digest_buffer(
            self._exec, self.handle, C.byref(num_groups), C.byref(num_worlds)) or 0)
        assert num_worlds.value == self.num_worlds
        # the archetype names, from the plan column that opens each group
        self.groups = []
        for g in range(num_groups.value):
            arch, tag = C.c_uint32(0), C.c_uint32(0)
            self._check(self._rt.mwhip_digest_group(self._exec, self.handle, g,
                                                    C.byref(arch), C.byref(tag)),
                        "mwhip_digest_group")
            self.groups.append(self._tables[tag.value])

    def _live(self) -> int:
        handle = super()._live()
        if self._rt is None:
            raise RuntimeError("only compute() works on the reference backend: "
                               "this needs the HIP backend")
        return handle

    def compute(self) -> np.ndarray:
        """uint64 [groups, worlds]; waits for the executor's stream."""
        if self._rt is None:
            super()._live()
            sim = self._sim
            return digest_ref.digest_of_dump(
                self._tables, [sim.dump_column(i) for i in self._indices], self.num_worlds)
        _Computed.compute(self)
        return self.read()

    def read(self) -> np.ndarray:
        """The device buffer as it is (what the last compute, compute_async or
        step left), uint64 [groups, worlds]; waits for the executor's stream."""
        self._live()
        self._sim.sync()
        return self.tensor.cpu().numpy().view(np.uint64)

    @property
    def tensor(self):
        """torch int64 [groups, worlds] over the device buffer (no copy)."""
        self._live()
        return self._wrap("tensor", self.buffer_ptr, np.int64,
                          (len(self.groups), self.num_worlds))

    def _step_args(self, handle: int, on: bool) -> tuple:
        # (the executor has one step digest: set by its handle, unset by 0)
        return (handle if on else 0,)


class _WorldColumns(_Cells):
    """What WorldView and WorldWrite share: columns of ONE table, named as the
    dump list names them, per column a device buffer of [worlds, max_rows]
    cells, and int32 [worlds] counts."""

    _what = ""      # in messages

    def __init__(self, sim: "Simulator", table: str, columns, max_rows: int):
        names, of_table = _table_columns(sim, table, self._what)
        _need_column_ids(sim)
        if columns is None:
            columns = self._default_columns(sim, names, of_table)
        columns = list(columns)
        for name in columns:
            if name not in of_table:
                raise KeyError(f"{self._what}: {name!r} is not a column of table {table!r}")
        if not columns:
            raise ValueError(f"{self._what}: no columns")
        if len(set(columns)) != len(columns):
            raise ValueError(f"{self._what}: a column is listed twice")
        self._open(sim)
        self.table = table
        self.columns = columns
        self.max_rows = int(max_rows)
        self.num_worlds = sim.num_worlds
        self.archetype, comps = _one_table(sim, names, columns)
        self._create(self.archetype, (C.c_uint32 * len(comps))(*comps), len(comps),
                     min(max(self.max_rows, 0), 0xFFFFFFFF))
        self._open_buffers(columns)
        self.counts_ptr = self._pointer("counts")

    @staticmethod
    def _default_columns(sim, names, of_table):
        return of_table

    def _shape(self) -> tuple:
        return self.num_worlds, self.max_rows

    @property
    def counts(self):
        """torch int32 [worlds] over the device buffer (no copy): each world's
        rows in the table as the last compute or apply found them, which may
        exceed max_rows."""
        return self._int32("counts", self.counts_ptr, self.num_worlds)


class WorldView(_Computed, _WorldColumns):
    """A dense, zero-padded, world-major copy of columns of ONE table on the
    device: per column uint8 [worlds, max_rows, cell_bytes], plus int32 [worlds]
    row counts that are NOT clipped to max_rows (counts[w] > max_rows: rows were
    dropped).  madrona_amd/view_ref.py is the exact definition; mwhip_view_*,
    include/mwhip.h, computes it with one kernel where the table is, sorted or
    not.  HIP backend only.  compute() waits for the executor's stream,
    compute_async() queues behind the replays queued so far; tensor(name) and
    `counts` are zero-copy torch tensors over the device buffers, which every
    compute rewrites in full; every_step() makes every replay of a step graph
    recompute the view (before its output rings: a ring over buffer_ptr(name)
    records [K, worlds, max_rows, ...]).  close() frees it; Simulator.close()
    orphans what is left."""

    _kind, _stem, _list = "world view", "view", "_views"
    _what = "world_view()"

    def handle_source(self, name: str, first_byte: int = 0, handles: int = 1):
        """The slab of column `name` as a source of Simulator.entity_gather():
        (ptr, num_records, record_bytes, first_byte, handles_per_record) with a
        record per cell, worlds * max_rows of them, and in each `handles`
        Entity cells from byte `first_byte` on.  The padding cells are records
        like any other (zero handles, whatever those name)."""
        ptr, cell = self._buffers[name]
        self._live()
        if first_byte < 0 or handles < 1 or first_byte + 8 * handles > cell:
            raise ValueError(f"{name}: {handles} handles from byte {first_byte} do not fit "
                             f"cells of {cell} bytes")
        return (ptr, self.num_worlds * self.max_rows, cell, int(first_byte), int(handles))


class WorldWrite(_Applied, _WorldColumns):
    """The inverse of a WorldView: tensors on the device that are scattered
    into columns of ONE table.  Per column uint8 [worlds, max_rows, cell_bytes]
    (tensor(name): exactly the layout of a WorldView of the same columns and
    max_rows, so a view's tensors can be copied in one for one) and int32
    [worlds] `take`; apply() makes the listed cells of the first
    min(max(take[w], 0), rows of w, max_rows) rows of every world w, in table
    order, those of the tensors, and leaves each world's row count, not
    clipped, in `counts`.  Nothing else of the table changes, Entity and
    WorldID cannot be listed, and what the simulator derives from a written
    component follows when its own systems next derive it.
    madrona_amd/write_ref.py is the exact definition; mwhip_write_*,
    include/mwhip.h, applies it with one kernel where the table is, sorted or
    not.  HIP backend only.  All buffers start as zeros (take too: nothing is
    written until it is set).

    apply() waits for the executor's stream, apply_async() queues behind the
    replays queued so far.  FILLING THE TENSORS IS THE CALLER'S TO ORDER: torch
    fills them on its own stream, so synchronize that stream (or make the
    executor's stream wait for it) before apply_async() or a step that carries
    the write, exactly as for the exported action tensors.  every_step() makes
    every replay of a step graph apply the write behind its input rings and in
    front of its first node: an input ring over buffer_ptr(name) or take_ptr
    feeds K queued steps K different injections.  close() frees it;
    Simulator.close() orphans what is left."""

    _kind, _stem, _list = "world write", "write", "_writes"
    _what = "world_write()"

    def __init__(self, sim: "Simulator", table: str, columns, max_rows: int):
        super().__init__(sim, table, columns, max_rows)
        self._take_ptr = self._pointer("take")

    @staticmethod
    def _default_columns(sim, names, of_table):
        # (component 0 is Entity, 1 is WorldID: include/mwhip.h)
        return [n for n in of_table if _column_ids(sim, names.index(n), n)[1] not in (0, 1)]

    @property
    def take_ptr(self) -> int:
        """Device address of the int32 [worlds] take buffer."""
        self._live()
        return self._take_ptr

    @property
    def take(self):
        """torch int32 [worlds] over the device buffer (no copy): the leading
        rows of each world to write.  The caller fills it."""
        return self._int32("take", self._take_ptr, self.num_worlds)


class WorldReduce(_Computed, _StepObject):
    """One number per world, element and term about ONE table, on the device:
    per term a [worlds, elems] tensor of sums, minima, maxima, largest
    magnitudes, counts of non-zero or of non-finite values over each world's
    rows in table order, plus int32 [worlds] `counts` (each world's rows) and
    int32 [worlds] `alarm` (1 where a term made with alarm=True trips).
    madrona_amd/reduce_ref.py is the exact definition, the order of the float
    sum included; mwhip_reduce_*, include/mwhip.h, computes it with one kernel
    where the table is, sorted or not.  HIP backend only.

    A term is (column, op) or (column, op, options): op one of "sum", "min",
    "max", "absmax", "count_nonzero", "count_nonfinite"; options a dict of
    dtype ("f32", "i32", "u32", "u8"; default f32 for a float column, else u32
    for cells of whole dwords, else u8), offset (bytes into the cell, default
    0), elems (default: the rest of the cell), limit and alarm.  `terms` holds
    them as (column, reduce_ref.Term).

    compute() waits for the executor's stream, compute_async() queues behind
    the replays queued so far; every compute rewrites every buffer in full.
    every_step() makes every replay of a step graph recompute the reduce
    (behind its step views, before its output rings: a ring over buffer_ptr(i)
    records [K, worlds, elems]; an input ring of one slot over alarm_ptr feeds
    this step's alarms to the next queued step).  close() frees it;
    Simulator.close() orphans what is left."""

    _kind, _stem, _list = "world reduce", "reduce", "_reduces"

    def __init__(self, sim: "Simulator", table: str, terms):
        from . import reduce_ref

        info = {c[0]: c for c in sim._columns}
        names, of_table = _table_columns(sim, table, "world_reduce()")
        _need_column_ids(sim)
        terms = list(terms)
        if not terms:
            raise ValueError("world_reduce(): no terms")
        self.terms = []
        for given in terms:
            column, op = given[0], given[1]
            options = dict(given[2]) if len(given) > 2 else {}
            if column not in of_table:
                raise KeyError(f"world_reduce(): {column!r} is not a column of table {table!r}")
            if op not in reduce_ref.OPS:
                raise ValueError(f"world_reduce(): unknown op {op!r}")
            _, cell, is_float = info[column]
            dtype = options.pop("dtype", None)
            if dtype is None:
                dtype = "f32" if is_float else ("u32" if cell % 4 == 0 else "u8")
            if dtype not in reduce_ref.DTYPES:
                raise ValueError(f"world_reduce(): unknown dtype {dtype!r}")
            item = 1 if dtype == "u8" else 4
            offset = int(options.pop("offset", 0))
            elems = options.pop("elems", None)
            if elems is None:
                elems = max(cell - offset, 0) // item
            term = reduce_ref.Term(op, dtype, offset, int(elems),
                                   float(options.pop("limit", 0.0)),
                                   bool(options.pop("alarm", False)))
            if options:
                raise TypeError(f"world_reduce(): unknown options {sorted(options)}")
            self.terms.append((column, term))
        self._open(sim)
        self.table = table
        self.num_worlds = sim.num_worlds
        self.archetype, comps = _one_table(sim, names, [column for column, _ in self.terms])
        arr = (ReduceTerm * len(self.terms))(*[
            ReduceTerm(comp, min(max(term.offset, 0), 0xFFFFFFFF),
                       min(max(term.elems, 0), 0xFFFFFFFF),
                       reduce_ref.DTYPES[term.dtype], reduce_ref.OPS[term.op],
                       reduce_ref.ALARM if term.alarm else 0, term.limit)
            for comp, (_, term) in zip(comps, self.terms)])
        self._create(self.archetype, arr, len(self.terms))
        self._buffers = []
        for p, (_, term) in enumerate(self.terms):
            nbytes, elems = C.c_uint64(0), C.c_uint32(0)
            ptr = self._rt.mwhip_reduce_buffer(self._exec, self.handle, p, C.byref(nbytes),
                                               C.byref(elems))
            assert ptr and elems.value == term.elems and \
                nbytes.value == self.num_worlds * term.elems * 4
            self._buffers.append((int(ptr), reduce_ref.result_dtype(term)))
        self.counts_ptr = self._pointer("counts")
        self._alarm_ptr = self._pointer("alarm")

    def buffer_ptr(self, i: int) -> int:
        """Device address of term i's [worlds, elems] results (4 bytes each)."""
        self._live()
        return self._buffers[i][0]

    @property
    def alarm_ptr(self) -> int:
        """Device address of the int32 [worlds] alarm buffer."""
        self._live()
        return self._alarm_ptr

    def tensor(self, i: int):
        """torch [worlds, elems] over the device buffer of term i (no copy) in
        the result type: float32, int32 or uint32."""
        self._live()
        ptr, dtype = self._buffers[i]
        return self._wrap((i, dtype.str), ptr, dtype.type,
                          (self.num_worlds, self.terms[i][1].elems))

    @property
    def counts(self):
        """torch int32 [worlds] over the device buffer (no copy): each world's
        rows in the table as the last compute found them."""
        return self._int32("counts", self.counts_ptr, self.num_worlds)

    @property
    def alarm(self):
        """torch int32 [worlds] over the device buffer (no copy): 1 where an
        alarm term tripped in the last compute, else 0."""
        return self._int32("alarm", self._alarm_ptr, self.num_worlds)


class _HandleCells(_Cells):
    """What EntityGather and EntityScatter share: a source of N handles, a list
    of components named as the dump list names them, per component a device
    buffer of N cells, and int32 [N] archetypes and worlds."""

    _what = "entity_gather()"   # in messages

    def __init__(self, sim: "Simulator", source, components):
        comps, components = self._component_list(sim, components)
        # (a tensor stays where it is while the object exists)
        self._source, ptr, num_records, record_bytes, first_byte, per = \
            self._handle_source(source)
        self._open(sim)
        self.components = components
        self.num_handles = num_records * per
        src = GatherSource(ptr, num_records, record_bytes, first_byte, per, 0)
        self._create(C.byref(src), comps, len(components))
        self._open_buffers(components)
        self.archetypes_ptr = self._pointer("archetypes")
        self.worlds_ptr = self._pointer("worlds")

    def _shape(self) -> tuple:
        return (self.num_handles,)

    @classmethod
    def _component_list(cls, sim: "Simulator", components):
        """(the component ids as a C array, the names as a list)"""
        _need_column_ids(sim)
        components = list(components)
        if len(set(components)) != len(components):
            raise ValueError(f"{cls._what}: a component is listed twice")
        comps = (C.c_uint32 * max(len(components), 1))()
        for p, name in enumerate(components):
            comps[p] = cls._component_id(sim, name)
        return comps, components

    @classmethod
    def _handle_source(cls, source):
        """(the tensor to keep alive or None, ptr, num_records, record_bytes,
        first_byte, handles_per_record) of a source as entity_gather() and
        entity_scatter() take it"""
        if isinstance(source, tuple):
            return (None,) + tuple(int(v) for v in source)
        import torch

        four_byte = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())
        if not isinstance(source, torch.Tensor) or not source.is_cuda:
            raise TypeError(f"{cls._what}: the source is a torch tensor on the device or "
                            "a (ptr, num_records, record_bytes, first_byte, "
                            "handles_per_record) tuple")
        if not ((source.dtype in four_byte and source.dim() >= 1 and source.shape[-1] == 2)
                or (source.dtype == torch.uint8 and source.dim() >= 1
                    and source.shape[-1] == 8)):
            raise TypeError(f"{cls._what}: handles are int32 / uint32 [..., 2] or uint8 "
                            f"[..., 8], not {source.dtype} {tuple(source.shape)}")
        if not source.is_contiguous():
            raise ValueError(f"{cls._what}: the source tensor must be contiguous")
        return (source, source.data_ptr(), source.numel() * source.element_size() // 8,
                8, 0, 1)

    @classmethod
    def _component_id(cls, sim: "Simulator", name: str) -> int:
        """A component is named by the part of a dump-list column name behind
        the dot; every table's column of that name must be the same component."""
        ids = set()
        for idx, column in enumerate(sim._columns):
            if column[0].split(".", 1)[-1] != name:
                continue
            ids.add(_column_ids(sim, idx, column[0])[1])
        if not ids:
            raise KeyError(f"{cls._what}: no column of the dump list is named "
                           f"'<table>.{name}'")
        if len(ids) != 1:
            raise KeyError(f"{cls._what}: {name!r} names different components "
                           f"{sorted(ids)} in different tables")
        return ids.pop()

    def _orphan(self) -> None:
        super()._orphan()
        self._source = None

    @property
    def archetypes(self):
        """torch int32 [N] over the device buffer (no copy): the archetype of
        the entity each handle names, -1 where it names nothing."""
        return self._int32("archetypes", self.archetypes_ptr, self.num_handles)

    @property
    def worlds(self):
        """torch int32 [N] over the device buffer (no copy): the world of the
        entity each handle names, -1 where it names nothing."""
        return self._int32("worlds", self.worlds_ptr, self.num_handles)


class EntityGather(_Computed, _HandleCells):
    """The cells of the entities that N handles in device memory name: per
    listed component uint8 [N, cell_bytes] (zero where a handle names nothing
    or its table has no such column), plus int32 [N] `archetypes` and `worlds`
    (-1 where it names nothing).  madrona_amd/gather_ref.py is the exact
    definition; mwhip_gather_*, include/mwhip.h, computes it with one kernel
    through the entity store, trusting no bit of a handle.  HIP backend only.
    The source is read when the kernel runs and must stay where it is while the
    gather exists (a tensor given as the source is kept alive by this object).
    compute() waits for the executor's stream, compute_async() queues behind
    the replays queued so far; tensor(name), `archetypes` and `worlds` are
    zero-copy torch tensors over the device buffers, which every compute
    rewrites in full; every_step() makes every replay of a step graph recompute
    the gather directly behind its step views (so a gather over a step view's
    slab follows the step) and before its output rings: a ring over
    buffer_ptr(name) records [K, N, ...].  close() frees it; Simulator.close()
    orphans what is left."""

    _kind, _stem, _list = "entity gather", "gather", "_gathers"


class EntityScatter(_Applied, _HandleCells):
    """The batched ctx.get<T>(e) = v: per listed component a device buffer of N
    cells (tensor(name), uint8 [N, cell_bytes]) and int32 [N] `select`, filled
    by the caller; apply() stores cell i into the entity that handle i of the
    source names, for every i with select[i] != 0, and among selected handles
    that name the same entity the highest index wins, as `column[rows] = values`
    assigned one at a time would.  int32 [N] `archetypes`, `worlds` (-1 where a
    handle names nothing) and `written` (1 where handle i's cells are the ones
    now in the table) are rewritten by every apply.  madrona_amd/scatter_ref.py
    is the exact definition; mwhip_scatter_*, include/mwhip.h, computes it with
    three launches through the entity store, trusting no bit of a handle.  The
    other direction of an EntityGather, with the same sources (a tensor given as
    the source is kept alive by this object).  Entity and WorldID cannot be
    listed; no rows are made or destroyed; what the simulator derives from the
    cells written is its own business.  HIP backend only.  apply() waits for the
    executor's stream, apply_async() queues behind the replays queued so far;
    every_step() makes every replay of a step graph apply the scatter directly
    behind its step writes and in front of its first node, so an input ring
    into buffer_ptr(name), select_ptr or the caller's handle tensor feeds the
    apply of the replay it runs in.  Step scatters list disjoint components.
    close() frees it; Simulator.close() orphans what is left."""

    _kind, _stem, _list = "entity scatter", "scatter", "_scatters"
    _what = "entity_scatter()"

    def __init__(self, sim: "Simulator", source, components):
        super().__init__(sim, source, components)
        self.select_ptr = self._pointer("select")
        self.written_ptr = self._pointer("written")

    @property
    def select(self):
        """torch int32 [N] over the device buffer (no copy), the caller's to
        fill: handle i's cells are stored where it is non-zero."""
        return self._int32("select", self.select_ptr, self.num_handles)

    @property
    def written(self):
        """torch int32 [N] over the device buffer (no copy): 1 where the last
        apply stored handle i's cells (selected, names an entity, and no
        selected handle of higher index names the same one)."""
        return self._int32("written", self.written_ptr, self.num_handles)


class _Sourced:
    """What RayQuery, BoxQuery, ContactQuery and ShapeQuery share: inputs that may be read
    from the caller's source (mwhip_ray_source)."""

    _what = ""      # in messages

    @classmethod
    def _source(cls, what: str, source, item_bytes: int):
        """(the tensor to keep alive or None, RaySource) of None, a device
        tensor whose rows are the records, or (ptr, record_bytes, first_byte)"""
        if source is None:
            return None, RaySource(None, 0, 0)
        if isinstance(source, tuple):
            ptr, record_bytes, first_byte = (int(v) for v in source)
            return None, RaySource(ptr, record_bytes, first_byte)
        import torch

        if not isinstance(source, torch.Tensor) or not source.is_cuda:
            raise TypeError(f"{cls._what}: {what} is a torch tensor on the device or a "
                            "(ptr, record_bytes, first_byte) tuple")
        if source.element_size() != 4 or not source.is_contiguous() or source.dim() < 1:
            raise TypeError(f"{cls._what}: the {what} tensor must be contiguous with 4-byte "
                            f"items, not {source.dtype} {tuple(source.shape)}")
        record = item_bytes if source.dim() == 1 else int(source.shape[-1]) * 4
        if record < item_bytes:
            raise TypeError(f"{cls._what}: rows of {record} bytes are too short for {what}")
        return source, RaySource(source.data_ptr(), record, 0)


class _TreeQuery(_Computed, _Sourced, _StepObject):
    """What RayQuery and BoxQuery share: groups (fans, bundles) that each have a
    world and a point (origin, centre), either in a buffer the query owns or
    read from the caller's source, and buffers asked for by name
    (mwhip_<stem>_buffer, _BUFS)."""

    _BUFS: Dict[str, int] = {}
    _PER_WORLD = ("", "")       # the constructor's groups-per-world argument, a group

    def _open_query(self, sim: "Simulator", desc, world, count, point: str, given,
                    per_world: int) -> None:
        """desc: the descriptor with its numbers filled in; point: its field
        (and the buffer) of the groups' points, `given` the caller's source"""
        self._open(sim)
        keep_w, desc.world = self._source("world", world, 4)
        keep_c, desc.count = self._source("count", count, 4)
        keep_o, source = self._source(point, given, 12)
        setattr(desc, point, source)
        self._sources = (keep_w, keep_c, keep_o)    # (stay where they are)
        self._create(C.byref(desc))
        self._per_world = per_world
        self._owned = {"world": world is None and per_world == 0, point: given is None}

    def _orphan(self) -> None:
        super()._orphan()
        self._sources = ()

    def buffer_ptr(self, name: str) -> int:
        """Device address of owned buffer `name` (a key of _BUFS)."""
        handle = self._live()
        nbytes = C.c_uint64(0)
        what = f"mwhip_{self._stem}_buffer"
        ptr = getattr(self._rt, what)(self._exec, handle, self._BUFS[name], C.byref(nbytes))
        if not ptr:
            raise RuntimeError(f"{what}({name}): {self._rt.mwhip_last_error().decode()}")
        return int(ptr)

    def _tensor(self, name, dtype, shape):
        self._live()
        if not self._owned.get(name, True):
            per_world, group = self._PER_WORLD
            raise RuntimeError(f"this {self._kind} owns no {name} buffer: " + (
                f"{per_world} gives each {group} its world" if name == "world"
                and self._per_world else f"a {name} source was given"))
        if name not in self._tensors:
            self._wrap(name, self.buffer_ptr(name), dtype, shape)
        return self._tensors[name]


class RayQuery(_TreeQuery):
    """N = fans x rays_per_fan rays cast through the worlds' broadphase BVHs by
    one kernel (mwhip_rays_*, include/mwhip.h; madrona_amd/ray_ref.py is the
    exact definition).  The rays of a fan share an origin and a world.  Inputs:
    worlds() int32 [F], origins() float32 [F, 3] (each owned unless a source
    was given -- a device tensor or (ptr, record_bytes, first_byte), read when
    the kernel runs and kept in place while the query exists; fans_per_world >
    0 replaces worlds() by world = f // fans_per_world, and `count`, an int32
    per world such as a view's counts, then SKIPS fans f % fans_per_world >=
    count[world]), directions() float32 [N, 3] (used as given) and t_max()
    float32 [N] (+inf at creation).  Outputs, rewritten in full by every
    compute: status() int32 [N] (HIT 1, MISS 0, SKIPPED -1, BAD_WORLD -2,
    BAD_RAY -3), hit_t() float32 [N], hits() int32 [N, 2] (gen, id;
    Entity::none() = -1, -1 on anything but a hit), normals() float32 [N, 3].
    All are zero-copy torch tensors over the device buffers; what torch writes
    into the inputs on its own stream must have landed before a compute or a
    step reads it (torch.cuda.synchronize(): the executor's stream is
    non-blocking, the ordering is the caller's).  A world whose tree no
    broadphase pass has built yet (before its first step) gives MISS.  A ray sees the
    tree as the last broadphase pass of the step left it; spheres are
    transparent.  handle_source() is what entity_gather() / entity_scatter()
    take to go from hits to cells.  compute() waits for the executor's stream,
    compute_async() queues behind the replays queued so far; every_step() makes
    every replay of a step graph recompute the query behind its step views and
    in front of its step gathers and output rings.  HIP backend only."""

    _kind, _stem, _list = "ray query", "rays", "_ray_queries"
    HIT, MISS, SKIPPED, BAD_WORLD, BAD_RAY = 1, 0, -1, -2, -3
    _BUFS = {"world": 0, "origin": 1, "dir": 2, "t_max": 3, "hit_t": 4, "hit": 5, "normal": 6,
             "status": 7}
    _what, _PER_WORLD = "ray_query()", ("fans_per_world", "fan")

    def __init__(self, sim: "Simulator", fans: int, rays_per_fan: int, world=None, origin=None,
                 fans_per_world: int = 0, count=None):
        self.num_fans, self.rays_per_fan = int(fans), int(rays_per_fan)
        self.num_rays = self.num_fans * self.rays_per_fan
        self.fans_per_world = int(fans_per_world)
        desc = RaysDesc(self.num_fans, self.rays_per_fan, self.fans_per_world, 0)
        self._open_query(sim, desc, world, count, "origin", origin, self.fans_per_world)

    def worlds(self):
        """int32 [F] (owned: no world source and no fans_per_world)"""
        return self._tensor("world", np.int32, (self.num_fans,))

    def origins(self):
        """float32 [F, 3] (owned: no origin source)"""
        return self._tensor("origin", np.float32, (self.num_fans, 3))

    def directions(self):
        """float32 [N, 3]"""
        return self._tensor("dir", np.float32, (self.num_rays, 3))

    def t_max(self):
        """float32 [N], +inf at creation"""
        return self._tensor("t_max", np.float32, (self.num_rays,))

    def hit_t(self):
        """float32 [N], 0 on anything but a hit"""
        return self._tensor("hit_t", np.float32, (self.num_rays,))

    def hits(self):
        """int32 [N, 2] (gen, id), -1, -1 on anything but a hit"""
        return self._tensor("hit", np.int32, (self.num_rays, 2))

    def normals(self):
        """float32 [N, 3], zero on anything but a hit"""
        return self._tensor("normal", np.float32, (self.num_rays, 3))

    def status(self):
        """int32 [N]: HIT 1, MISS 0, SKIPPED -1, BAD_WORLD -2, BAD_RAY -3"""
        return self._tensor("status", np.int32, (self.num_rays,))

    def handle_source(self):
        """The hits as a source of Simulator.entity_gather() / entity_scatter():
        (ptr, num_records, record_bytes, first_byte, handles_per_record)."""
        return (self.buffer_ptr("hit"), self.num_rays, 8, 0, 1)


class BoxQuery(_TreeQuery):
    """B = bundles x boxes_per_bundle boxes tested through the worlds' broadphase
    BVHs by one kernel: per box the whole list of the entities
    PhysicsSystem::findEntitiesWithinAABB reports, in the order it reports them
    (mwhip_boxes_*, include/mwhip.h; madrona_amd/box_ref.py is the exact
    definition).  The boxes of a bundle share a world and a centre: box b = f *
    G + g is pMin = centre[f] + lo[b], pMax = centre[f] + hi[b] in float32.
    Inputs: worlds() int32 [F], centres() float32 [F, 3] (each owned unless a
    source was given -- a device tensor or (ptr, record_bytes, first_byte),
    read when the kernel runs and kept in place while the query exists;
    bundles_per_world > 0 replaces worlds() by world = f // bundles_per_world,
    and `count`, an int32 per world such as a view's counts, then SKIPS bundles
    f % bundles_per_world >= count[world]), lo() and hi() float32 [B, 3].  All
    owned inputs are zero at creation: empty boxes, and with owned centres lo
    and hi are absolute corners.  Outputs, rewritten in full by every compute:
    status() int32 [B] (OK 0, SKIPPED -1, BAD_WORLD -2, BAD_BOX -3), counts()
    int32 [B] (not capped by max_hits, 0 unless OK), hits() int32 [B, K, 2]
    (gen, id): the first min(count, K) entities, -1, -1 behind them.  All are
    zero-copy torch tensors over the device buffers; what torch writes into the
    inputs on its own stream must have landed before a compute or a step reads
    it (torch.cuda.synchronize()).  A world whose tree no broadphase pass has
    built yet (before its first step) gives OK with count 0.  A box sees the
    tree as the last broadphase pass of the step left it and the poses as they
    are now.  handle_source() is what entity_gather() / entity_scatter() take
    to go from hits to cells.  packed=True maps a box to a lane through plain
    findEntitiesWithinAABB instead of a chunk of a bundle to a group of 32
    lanes; same words.  compute() waits for the executor's stream,
    compute_async() queues behind the replays queued so far; every_step() makes
    every replay of a step graph recompute the query behind its step views and
    ray queries and in front of its step gathers and output rings.  HIP backend
    only."""

    _kind, _stem, _list = "box query", "boxes", "_box_queries"
    OK, SKIPPED, BAD_WORLD, BAD_BOX = 0, -1, -2, -3
    PACKED = 1
    _BUFS = {"world": 0, "centre": 1, "lo": 2, "hi": 3, "status": 4, "count": 5, "hits": 6}
    _what, _PER_WORLD = "box_query()", ("bundles_per_world", "bundle")

    def __init__(self, sim: "Simulator", bundles: int, boxes_per_bundle: int, max_hits: int,
                 world=None, centre=None, bundles_per_world: int = 0, count=None,
                 packed: bool = False):
        self.num_bundles, self.boxes_per_bundle = int(bundles), int(boxes_per_bundle)
        self.max_hits = int(max_hits)
        self.num_boxes = self.num_bundles * self.boxes_per_bundle
        self.bundles_per_world = int(bundles_per_world)
        self.packed = bool(packed)
        desc = BoxesDesc(self.num_bundles, self.boxes_per_bundle, self.max_hits,
                         self.bundles_per_world, self.PACKED if self.packed else 0, 0)
        self._open_query(sim, desc, world, count, "centre", centre, self.bundles_per_world)

    def worlds(self):
        """int32 [F] (owned: no world source and no bundles_per_world)"""
        return self._tensor("world", np.int32, (self.num_bundles,))

    def centres(self):
        """float32 [F, 3] (owned: no centre source)"""
        return self._tensor("centre", np.float32, (self.num_bundles, 3))

    def lo(self):
        """float32 [B, 3]: pMin = centre + lo"""
        return self._tensor("lo", np.float32, (self.num_boxes, 3))

    def hi(self):
        """float32 [B, 3]: pMax = centre + hi"""
        return self._tensor("hi", np.float32, (self.num_boxes, 3))

    def status(self):
        """int32 [B]: OK 0, SKIPPED -1, BAD_WORLD -2, BAD_BOX -3"""
        return self._tensor("status", np.int32, (self.num_boxes,))

    def counts(self):
        """int32 [B]: the entities the box holds, not capped by max_hits"""
        return self._tensor("count", np.int32, (self.num_boxes,))

    def hits(self):
        """int32 [B, K, 2] (gen, id), -1, -1 behind the first min(count, K)"""
        return self._tensor("hits", np.int32, (self.num_boxes, self.max_hits, 2))

    def handle_source(self):
        """The hits as a source of Simulator.entity_gather() / entity_scatter():
        (ptr, num_records, record_bytes, first_byte, handles_per_record)."""
        return (self.buffer_ptr("hits"), self.num_boxes * self.max_hits, 8, 0, 1)


class ContactQuery(_Computed, _Sourced, _StepObject):
    """Per world the primitive pairs of its rigid bodies that touch, with the
    manifold the physics step's narrowphase builds for each: which bodies, where,
    how deep (mwhip_contacts_*, include/mwhip.h; madrona_amd/contact_ref.py is
    the exact definition).  The bodies of a world are the rows of its rigid-body
    tables in the step's order; every pair of them that is not Static-Static and
    every primitive pair of the two objects is tested, the body of lower entity
    id as `a`; a pair is a contact iff the primitives' world boxes intersect and
    the narrowphase returns at least one point.  Contacts come in the order
    (k_lo, k_hi, primitive pair).  No BVH is walked.
    poses="solver" (the default, XPBD simulators only) takes each body where the
    solver's last substep built its contacts (xpbd::PreSolvePositional), where a
    resting body penetrates by about g h^2 and a resting contact does not
    flicker; a body never stepped since it was created is taken as it is.
    poses="current" takes Position and Rotation as they are now, e.g. right
    after a world write.  Input: selects() int32 [W] if select=True (owned, 1 at
    creation), or `select` a device tensor / (ptr, record_bytes, first_byte)
    read when the kernel runs; 0 skips the world.  Outputs, rewritten in full by
    every compute, zero-copy torch tensors: status() int32 [W] (OK 0, SKIPPED
    -1, UNSORTED -2, UNSUPPORTED -3), counts() int32 [W] (not capped by K, 0
    unless OK), pairs() int32 [W, K, 2, 2] ((gen, id) of the body that owns the
    reference feature, then of the other; -1, -1 behind min(count, K)),
    num_points() int32 [W, K], normals() float32 [W, K, 3], points() float32 [W,
    K, 4, 4] (xyz world position, w depth; zero from num_points on and behind
    min(count, K)).  handle_source() is what entity_gather() / entity_scatter()
    take to go from pairs to cells.  plain=True sends every pair through the
    generic single-lane routine, one at a time: the same words, slowly.
    compute() waits for the executor's stream, compute_async() queues behind the
    replays queued so far; every_step() makes every replay of a step graph
    recompute the query behind its step box queries and in front of its step
    gathers and output rings.  HIP backend only."""

    _kind, _stem, _list = "contact query", "contacts", "_contact_queries"
    OK, SKIPPED, UNSORTED, UNSUPPORTED = 0, -1, -2, -3
    CURRENT_POSES, PLAIN = 1, 2
    _BUFS = {"select": 0, "status": 1, "count": 2, "pairs": 3, "num_points": 4, "normal": 5,
             "points": 6}
    _what = "contact_query()"

    def __init__(self, sim: "Simulator", max_contacts: int, select=None, poses: str = "solver",
                 plain: bool = False):
        if poses not in ("solver", "current"):
            raise ValueError(f'contact_query(): poses is "solver" or "current", not {poses!r}')
        self.max_contacts = int(max_contacts)
        self.poses, self.plain = poses, bool(plain)
        self.num_worlds = sim.num_worlds
        self._open(sim)
        own = select is True
        self._source_kept, source = self._source("select", None if own else select, 4)
        desc = ContactsDesc(self.max_contacts,
                            (self.CURRENT_POSES if poses == "current" else 0) |
                            (self.PLAIN if self.plain else 0), 1 if own else 0, 0, source)
        self._create(C.byref(desc))
        self._owns_select = own

    def _orphan(self) -> None:
        super()._orphan()
        self._source_kept = None

    def buffer_ptr(self, name: str) -> int:
        """Device address of owned buffer `name` (a key of _BUFS)."""
        handle = self._live()
        nbytes = C.c_uint64(0)
        ptr = self._rt.mwhip_contacts_buffer(self._exec, handle, self._BUFS[name],
                                             C.byref(nbytes))
        if not ptr:
            raise RuntimeError(
                f"mwhip_contacts_buffer({name}): {self._rt.mwhip_last_error().decode()}")
        return int(ptr)

    def _tensor(self, name, dtype, shape):
        self._live()
        if name not in self._tensors:
            self._wrap(name, self.buffer_ptr(name), dtype, shape)
        return self._tensors[name]

    def selects(self):
        """int32 [W], 1 at creation (owned: select=True)"""
        if not self._owns_select:
            raise RuntimeError("this contact query owns no select buffer: make it with "
                               "select=True")
        return self._tensor("select", np.int32, (self.num_worlds,))

    def status(self):
        """int32 [W]: OK 0, SKIPPED -1, UNSORTED -2, UNSUPPORTED -3"""
        return self._tensor("status", np.int32, (self.num_worlds,))

    def counts(self):
        """int32 [W]: the world's contacts, not capped by max_contacts"""
        return self._tensor("count", np.int32, (self.num_worlds,))

    def pairs(self):
        """int32 [W, K, 2, 2]: (gen, id) of ref, then of alt; -1 behind min(count, K)"""
        return self._tensor("pairs", np.int32, (self.num_worlds, self.max_contacts, 2, 2))

    def num_points(self):
        """int32 [W, K]"""
        return self._tensor("num_points", np.int32, (self.num_worlds, self.max_contacts))

    def normals(self):
        """float32 [W, K, 3]"""
        return self._tensor("normal", np.float32, (self.num_worlds, self.max_contacts, 3))

    def points(self):
        """float32 [W, K, 4, 4]: xyz world position, w penetration depth"""
        return self._tensor("points", np.float32, (self.num_worlds, self.max_contacts, 4, 4))

    def handle_source(self):
        """The pairs as a source of Simulator.entity_gather() / entity_scatter():
        (ptr, num_records, record_bytes, first_byte, handles_per_record);
        handle 2 * (w * K + k) is contact k's ref, the next one its alt."""
        return (self.buffer_ptr("pairs"), self.num_worlds * self.max_contacts * 2, 8, 0, 1)


class ShapeQuery(_Computed, _Sourced, _StepObject):
    """"If this object stood THERE, what would it touch, where, and how deep?":
    S = bundles x shapes_per_bundle posed collision shapes, the shapes of a
    bundle in one world, each tested against the rigid bodies of its world with
    the physics step's narrowphase (mwhip_shapes_*, include/mwhip.h;
    madrona_amd/shape_ref.py is the exact definition).  Shape s = f * G + g is
    shape g of bundle f.  Inputs: worlds() int32 [F] and excludes() int32 [S, 2]
    (gen, id) -- each owned unless a source was given, a device tensor or (ptr,
    record_bytes, first_byte), read when the kernel runs and kept in place while
    the query exists; bundles_per_world > 0 replaces worlds() by world = f //
    bundles_per_world, and `count`, an int32 per world, then SKIPS bundles f %
    bundles_per_world >= count[world] --, and, always owned, objects() int32 [S]
    (an object of the simulator's ObjectManager, < num_objects), positions()
    float32 [S, 3], rotations() float32 [S, 4] (w, x, y, z) and scales() float32
    [S, 3]; at creation object 0 at the identity pose and unit scale in world 0,
    excluding nothing.  A body whose Entity equals a shape's exclude is not
    tested against it (the agent itself).  Every other body of the world, Static
    ones included, is tested at its CURRENT Position, Rotation and Scale, every
    primitive pair c = shapePrim * body_num_prims + bodyPrim of it, the shape as
    the step's `a`; a pair is a hit iff the primitives' world boxes intersect
    and the narrowphase returns at least one point.  Hits come in the order
    (body k, c).  No BVH is walked.  Outputs, rewritten in full by every compute,
    zero-copy torch tensors: status() int32 [S] (OK 0, SKIPPED -1, BAD_WORLD -2,
    BAD_SHAPE -3, UNSORTED -4, UNSUPPORTED -5), counts() int32 [S] (not capped by
    K, 0 unless OK), hits() int32 [S, K, 2] ((gen, id) of the body touched; -1,
    -1 behind min(count, K)), shape_is_ref() int32 [S, K] (1: the contact's
    reference side is the shape, and the normal points out of the shape; 0: out
    of the body), num_points() int32 [S, K], normals() float32 [S, K, 3],
    points() float32 [S, K, 4, 4] (xyz world position, w depth; zero from
    num_points on and behind min(count, K)).  What torch writes into the inputs
    on its own stream must have landed before a compute or a step reads it.
    handle_source() is what entity_gather() / entity_scatter() take to go from
    hits to cells.  plain=True sends every pair through the generic single-lane
    routine, one at a time: the same words.  compute() waits for the executor's
    stream, compute_async() queues behind the replays queued so far;
    every_step() makes every replay of a step graph recompute the query behind
    its step contact queries and in front of its step gathers and output rings.
    HIP backend only."""

    _kind, _stem, _list = "shape query", "shapes", "_shape_queries"
    OK, SKIPPED, BAD_WORLD, BAD_SHAPE, UNSORTED, UNSUPPORTED = 0, -1, -2, -3, -4, -5
    PLAIN = 1
    _BUFS = {"world": 0, "exclude": 1, "object": 2, "position": 3, "rotation": 4, "scale": 5,
             "status": 6, "count": 7, "hits": 8, "shape_is_ref": 9, "num_points": 10,
             "normal": 11, "points": 12}
    _what = "shape_query()"

    def __init__(self, sim: "Simulator", bundles: int, shapes_per_bundle: int, max_hits: int,
                 num_objects: int, world=None, bundles_per_world: int = 0, count=None,
                 exclude=None, plain: bool = False):
        self.num_bundles, self.shapes_per_bundle = int(bundles), int(shapes_per_bundle)
        self.num_shapes = self.num_bundles * self.shapes_per_bundle
        self.max_hits, self.num_objects = int(max_hits), int(num_objects)
        self.bundles_per_world, self.plain = int(bundles_per_world), bool(plain)
        self._open(sim)
        desc = ShapesDesc(self.num_bundles, self.shapes_per_bundle, self.max_hits,
                          self.num_objects, self.bundles_per_world,
                          self.PLAIN if self.plain else 0)
        keep_w, desc.world = self._source("world", world, 4)
        keep_c, desc.count = self._source("count", count, 4)
        keep_e, desc.exclude = self._source("exclude", exclude, 8)
        self._sources = (keep_w, keep_c, keep_e)    # (stay where they are)
        self._create(C.byref(desc))
        self._owned = {"world": world is None and self.bundles_per_world == 0,
                       "exclude": exclude is None}

    def _orphan(self) -> None:
        super()._orphan()
        self._sources = ()

    def buffer_ptr(self, name: str) -> int:
        """Device address of owned buffer `name` (a key of _BUFS)."""
        handle = self._live()
        nbytes = C.c_uint64(0)
        ptr = self._rt.mwhip_shapes_buffer(self._exec, handle, self._BUFS[name], C.byref(nbytes))
        if not ptr:
            raise RuntimeError(
                f"mwhip_shapes_buffer({name}): {self._rt.mwhip_last_error().decode()}")
        return int(ptr)

    def _tensor(self, name, dtype, shape):
        self._live()
        if not self._owned.get(name, True):
            raise RuntimeError(f"this shape query owns no {name} buffer: " + (
                "bundles_per_world gives each bundle its world" if name == "world"
                and self.bundles_per_world else f"a {name} source was given"))
        if name not in self._tensors:
            self._wrap(name, self.buffer_ptr(name), dtype, shape)
        return self._tensors[name]

    def worlds(self):
        """int32 [F] (owned: no world source and no bundles_per_world)"""
        return self._tensor("world", np.int32, (self.num_bundles,))

    def excludes(self):
        """int32 [S, 2]: (gen, id), -1, -1 (nothing) at creation (owned: no exclude source)"""
        return self._tensor("exclude", np.int32, (self.num_shapes, 2))

    def objects(self):
        """int32 [S]"""
        return self._tensor("object", np.int32, (self.num_shapes,))

    def positions(self):
        """float32 [S, 3]"""
        return self._tensor("position", np.float32, (self.num_shapes, 3))

    def rotations(self):
        """float32 [S, 4]: w, x, y, z"""
        return self._tensor("rotation", np.float32, (self.num_shapes, 4))

    def scales(self):
        """float32 [S, 3]"""
        return self._tensor("scale", np.float32, (self.num_shapes, 3))

    def status(self):
        """int32 [S]: OK 0, SKIPPED -1, BAD_WORLD -2, BAD_SHAPE -3, UNSORTED -4, UNSUPPORTED -5"""
        return self._tensor("status", np.int32, (self.num_shapes,))

    def counts(self):
        """int32 [S]: the shape's hits, not capped by max_hits"""
        return self._tensor("count", np.int32, (self.num_shapes,))

    def hits(self):
        """int32 [S, K, 2]: (gen, id) of the body touched; -1 behind min(count, K)"""
        return self._tensor("hits", np.int32, (self.num_shapes, self.max_hits, 2))

    def shape_is_ref(self):
        """int32 [S, K]: 1 where the contact's reference side is the shape"""
        return self._tensor("shape_is_ref", np.int32, (self.num_shapes, self.max_hits))

    def num_points(self):
        """int32 [S, K]"""
        return self._tensor("num_points", np.int32, (self.num_shapes, self.max_hits))

    def normals(self):
        """float32 [S, K, 3]"""
        return self._tensor("normal", np.float32, (self.num_shapes, self.max_hits, 3))

    def points(self):
        """float32 [S, K, 4, 4]: xyz world position, w penetration depth"""
        return self._tensor("points", np.float32, (self.num_shapes, self.max_hits, 4, 4))

    def handle_source(self):
        """The hits as a source of Simulator.entity_gather() / entity_scatter():
        (ptr, num_records, record_bytes, first_byte, handles_per_record)."""
        return (self.buffer_ptr("hits"), self.num_shapes * self.max_hits, 8, 0, 1)


class Simulator:
    """One simulator instance behind the C API (either backend)."""

    def __init__(self, lib_path: str, num_worlds: int, seed: int = 5,
                 gpu_id: int = 0, num_workers: int = 1, world_base: int = 0,
                 flags: int = 0):
        if not os.path.exists(lib_path):
            raise FileNotFoundError(
                f"{lib_path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        # RTLD_LOCAL: every simulator library defines the same C API (and
        # madronaMWHipUserEntry); they must not interpose on each other
        if lib_path.endswith("_hip.so"):
            _torch_runtime_first()
        self.lib = C.CDLL(lib_path, mode=C.RTLD_LOCAL)
        _bind(self.lib)
        self.num_worlds = num_worlds
        self.gpu_id = gpu_id
        args = SimCreateArgs(num_worlds, seed, gpu_id, num_workers, world_base, flags)
        self.handle = self.lib.sim_create(C.byref(args))
        if not self.handle:
            raise RuntimeError(f"sim_create failed for {lib_path}")
        self.backend = self.lib.sim_backend(self.handle).decode()
        self._async = None
        # what is open, a list per kind, named by the class's `_list`: _snapshots,
        # _digests, _views, _writes, _reduces, _gathers, _scatters, _ray_queries,
        # _box_queries, _contact_queries, _shape_queries; and _trajectories
        self._trajectories: List["Trajectory"] = []
        for name in _ExecObject._lists:
            setattr(self, name, [])
        self._tensor_info: Dict[str, Tuple[int, np.dtype, Tuple[int, ...], bool]] = {}
        for i in range(self.lib.sim_num_tensors(self.handle)):
            info = SimTensorInfo()
            self.lib.sim_tensor_info(self.handle, i, C.byref(info))
            dims = tuple(int(info.dims[k]) for k in range(info.ndim))
            self._tensor_info[info.name.decode()] = (
                i, np.dtype(SIM_DTYPES[info.dtype]), dims, bool(info.on_device))
        self._columns: List[Tuple[str, int, bool]] = []
        for i in range(self.lib.sim_num_columns(self.handle)):
            ci = SimColumnInfo()
            self.lib.sim_column_info(self.handle, i, C.byref(ci))
            self._columns.append((ci.name.decode(), int(ci.elem_bytes), bool(ci.is_float)))

    # -- lifecycle ---------------------------------------------------------
    def close(self) -> None:
        if self.handle:
            # sim_destroy frees the executor and with it every object of every
            # kind (what is left on _snapshots, _digests, _views, _writes,
            # _reduces, ...), and forgets its output rings (the trajectories
            # keep their tensors)
            for name in ["_trajectories", *_ExecObject._lists]:
                open_ones = getattr(self, name)
                for obj in open_ones:
                    obj._orphan()
                open_ones.clear()
            self.lib.sim_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, what: str) -> None:
        """(a call into the runtime: raises with its message)"""
        if rc != 0:
            raise RuntimeError(f"{what} -> {rc}: {runtime_lib().mwhip_last_error().decode()}")

    def step(self, n: int = 1) -> None:
        self.lib.sim_step(self.handle, n)

    # -- tensors -----------------------------------------------------------
    @property
    def tensor_names(self) -> List[str]:
        return list(self._tensor_info.keys())

    def tensor_meta(self, name: str):
        return self._tensor_info[name]

    def tensor_ptr(self, name: str) -> int:
        return int(self.lib.sim_tensor_ptr(self.handle, self._tensor_info[name][0]))

    def read_tensor(self, name: str) -> np.ndarray:
        idx, dtype, dims, _ = self._tensor_info[name]
        out = np.empty(dims, dtype=dtype)
        rc = self.lib.sim_tensor_read(self.handle, idx, out.ctypes.data, out.nbytes)
        if rc != 0:
            raise RuntimeError(f"sim_tensor_read({name}) -> {rc}")
        return out

    def write_tensor(self, name: str, value: np.ndarray) -> None:
        idx, dtype, dims, _ = self._tensor_info[name]
        arr = np.ascontiguousarray(value, dtype=dtype).reshape(dims)
        rc = self.lib.sim_tensor_write(self.handle, idx, arr.ctypes.data, arr.nbytes)
        if rc != 0:
            raise RuntimeError(f"sim_tensor_write({name}) -> {rc}")

    # -- parity dumps ------------------------------------------------------
    @property
    def columns(self) -> List[Tuple[str, int, bool]]:
        return list(self._columns)

    def dump_column(self, idx: int, max_rows_per_world: int = 256):
        name, elem_bytes, is_float = self._columns[idx]
        cap = self.num_worlds * max_rows_per_world * elem_bytes
        buf = np.empty(cap, dtype=np.uint8)
        counts = np.zeros(self.num_worlds, dtype=np.int32)
        n = self.lib.sim_column_dump(
            self.handle, idx, buf.ctypes.data, buf.nbytes,
            counts.ctypes.data_as(C.POINTER(C.c_int32)))
        if n < 0:
            detail = ""
            if self.backend == "hip":
                detail = ": " + runtime_lib().mwhip_last_error().decode()
            raise RuntimeError(f"sim_column_dump({name}) -> {n}{detail}")
        return buf[: n * elem_bytes].reshape(n, elem_bytes).copy(), counts

    def dump_all(self, max_rows_per_world: int = 256):
        return {self._columns[i][0]: self.dump_column(i, max_rows_per_world)
                for i in range(len(self._columns))}

    def run_taskgraph(self, taskgraph_id: int) -> None:
        """Replays ONE task graph of the simulator (HIP backend; test probes)."""
        rc = self.lib.sim_hip_run_taskgraph(self.handle, taskgraph_id)
        if rc != 0:
            raise RuntimeError(f"sim_hip_run_taskgraph({taskgraph_id}) -> {rc}")

    def taskgraph_graph(self, taskgraph_id: int) -> int:
        """Launch-graph handle of ONE task graph (the graph run_taskgraph
        replays; HIP backend), e.g. for profile(graph=...)."""
        fn = self.lib.sim_hip_taskgraph_graph
        fn.restype = C.c_uint64
        fn.argtypes = [C.c_void_p, C.c_uint32]
        g = int(fn(self.handle, taskgraph_id))
        if g == 0:
            raise RuntimeError(f"sim_hip_taskgraph_graph({taskgraph_id}) -> 0")
        return g

    def render(self) -> None:
        """MWCudaExecutor::buildRenderGraph + run: TLAS build and ray cast of every
        view into the simulator's "rgb" / "depth" tensors (HIP backend)."""
        self._check(self.lib.sim_hip_render(self.handle), "sim_hip_render")

    def render_graph(self) -> int:
        """Launch-graph handle of the render pass (for step_async(graph=...))."""
        return int(self.lib.sim_hip_render_graph(self.handle))

    def dump_column_raw(self, idx: int, max_rows: int):
        """Column `idx` in table order, destroyed rows included (HIP backend)."""
        name, elem_bytes, _ = self._columns[idx]
        buf = np.empty(max_rows * elem_bytes, dtype=np.uint8)
        n = self.lib.sim_column_dump_raw(self.handle, idx, buf.ctypes.data, buf.nbytes)
        if n < 0:
            raise RuntimeError(f"sim_column_dump_raw({name}) -> {n}")
        return buf[: n * elem_bytes].reshape(n, elem_bytes).copy()

    def hip_exec(self) -> int:
        return int(self.lib.sim_hip_exec(self.handle) or 0)

    def sort_stats(self) -> Dict[int, Dict[str, int]]:
        """Cumulative sort-node counters of every table that has been part of
        a sort node, by archetype id (mwhip_sort_stats; HIP backend): runs,
        stay_runs (compaction runs that patched the new rows in place),
        rows_copied (rows the gather copied per column), rows_in, rows_out,
        tail_rows, and of row reuse (mwhip_sort_reuse_stats) skipped_runs (world
        sorts that found every hole refilled in place and did nothing) and
        rows_reused.  Waits for the executor's stream."""
        rt = runtime_lib()
        rt.mwhip_sort_stats.restype = C.c_int32
        rt.mwhip_sort_stats.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(SortStats)]
        rt.mwhip_sort_reuse_stats.restype = C.c_int32
        rt.mwhip_sort_reuse_stats.argtypes = [C.c_void_p, C.c_uint32,
                                              C.POINTER(SortReuseStats)]
        out = {}
        archetype = 0
        while True:
            st = SortStats()
            rc = rt.mwhip_sort_stats(self.hip_exec(), archetype, C.byref(st))
            if rc == -1:
                return out
            if rc < 0:
                raise RuntimeError(f"mwhip_sort_stats({archetype}) -> {rc}")
            if rc == 0:
                out[archetype] = {name: int(getattr(st, name)) for name, _ in st._fields_}
                reuse = SortReuseStats()
                rc = rt.mwhip_sort_reuse_stats(self.hip_exec(), archetype, C.byref(reuse))
                if rc != 0:
                    raise RuntimeError(f"mwhip_sort_reuse_stats({archetype}) -> {rc}")
                out[archetype].update(skipped_runs=int(reuse.skipped_runs),
                                      rows_reused=int(reuse.rows_reused))
            archetype += 1

    def broadphase_stats(self, graph: int = 0) -> Dict[str, int]:
        """Replays of launch graph `graph` (default: the step graph) so far that
        left out the launches the simulator flagged as carried over
        (PhysicsSystem::BroadphaseInputs::CarriedOver), and replays that ran
        everything: {"carried_replays": n, "full_replays": m}
        (mwhip_broadphase_carry_stats; HIP backend).  Counted when a replay is
        queued; does not wait for the stream."""
        rt = runtime_lib()
        counters = (C.c_uint64 * 2)()
        rt.mwhip_broadphase_carry_stats.restype = C.c_int32
        rt.mwhip_broadphase_carry_stats.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        graph = graph or int(self.lib.sim_hip_step_graph(self.handle))
        rc = rt.mwhip_broadphase_carry_stats(self.hip_exec(), graph, counters)
        if rc != 0:
            raise RuntimeError(f"mwhip_broadphase_carry_stats({graph}) -> {rc}")
        return {"carried_replays": int(counters[0]), "full_replays": int(counters[1])}

    def _make(self, cls, needs: str, *args):
        """The factories' common part: cls(self, *args) on this simulator's
        list of them.  needs: who needs the HIP backend, "" for nobody."""
        if needs and self.backend != "hip":
            raise RuntimeError(f"{needs} the HIP backend, this is {self.backend!r}")
        obj = cls(self, *args)
        getattr(self, cls._list).append(obj)
        return obj

    def snapshot(self) -> "Snapshot":
        """A new, empty Snapshot of this simulator (HIP backend; raises on the
        reference backend, which has no executor to ask)."""
        return self._make(Snapshot, "snapshots need")

    def digest(self, columns=None) -> "StateDigest":
        """A StateDigest over `columns` of the dump list (names or indices, in
        that order; default: the whole dump list in its order).  Either
        backend: see StateDigest for what the reference backend offers."""
        return self._make(StateDigest, "", columns)

    def world_view(self, table: str, columns=None, max_rows: int = 0) -> "WorldView":
        """A WorldView of `columns` (names as in `columns`, e.g. "Item.Vec3";
        default: every dump-list column of the table) of table `table`, padded
        to max_rows rows per world.  HIP backend; raises on the reference
        backend, which has no executor to ask."""
        return self._make(WorldView, "world views need", table, columns, max_rows)

    def world_write(self, table: str, columns=None, max_rows: int = 0) -> "WorldWrite":
        """A WorldWrite into `columns` (names as in `columns`, e.g. "Item.Vec3";
        default: every dump-list column of the table except Entity and
        WorldID, which cannot be written) of table `table`, max_rows rows per
        world.  HIP backend; raises on the reference backend, which has no
        executor to ask."""
        return self._make(WorldWrite, "world writes need", table, columns, max_rows)

    def world_reduce(self, table: str, terms) -> "WorldReduce":
        """A WorldReduce of table `table`: one result per world and element for
        every term -- (column, op) or (column, op, options), see WorldReduce --
        plus each world's row count and an alarm word per world.  HIP backend;
        raises on the reference backend, which has no executor to ask."""
        return self._make(WorldReduce, "world reduces need", table, terms)

    def entity_gather(self, source, components) -> "EntityGather":
        """An EntityGather of `components` (named by the part of a dump-list
        column name behind the dot, e.g. "Position"; none: only archetypes and
        worlds) through the handles of `source`: a torch tensor on the device,
        contiguous, int32 / uint32 [..., 2] or uint8 [..., 8], or a (ptr,
        num_records, record_bytes, first_byte, handles_per_record) tuple such
        as WorldView.handle_source() gives.  HIP backend; raises on the
        reference backend, which has no executor to ask."""
        return self._make(EntityGather, "entity gathers need", source, components)

    def entity_scatter(self, source, components) -> "EntityScatter":
        """An EntityScatter of `components` (named as entity_gather() names
        them; at least one, neither Entity nor WorldID) through the handles of
        `source`, which takes every form entity_gather() takes,
        WorldView.handle_source() included.  HIP backend; raises on the
        reference backend, which has no executor to ask."""
        return self._make(EntityScatter, "entity scatters need", source, components)

    def ray_query(self, fans: int, rays_per_fan: int, world=None, origin=None,
                  fans_per_world: int = 0, count=None) -> "RayQuery":
        """A RayQuery of `fans` fans of `rays_per_fan` rays through the worlds'
        broadphase BVHs (HIP backend, a simulator with a broadphase).  `world`
        (int32 per fan), `origin` (3 floats per fan) and `count` (int32 per
        world, with fans_per_world) are device tensors whose rows are the
        records or (ptr, record_bytes, first_byte); None: world and origin are
        buffers the query owns (worlds(), origins()).  fans_per_world > 0:
        world = f // fans_per_world, the shape of a world view's slab.
        Simulator.close() frees what is left open."""
        return self._make(RayQuery, "ray queries need", fans, rays_per_fan, world, origin,
                          fans_per_world, count)

    def box_query(self, bundles: int, boxes_per_bundle: int, max_hits: int, world=None,
                  centre=None, bundles_per_world: int = 0, count=None,
                  packed: bool = False) -> "BoxQuery":
        """A BoxQuery of `bundles` bundles of `boxes_per_bundle` boxes through
        the worlds' broadphase BVHs, up to `max_hits` entities listed per box
        (HIP backend, a simulator with a broadphase).  `world` (int32 per
        bundle), `centre` (3 floats per bundle) and `count` (int32 per world,
        with bundles_per_world) are device tensors whose rows are the records
        or (ptr, record_bytes, first_byte); None: world and centre are buffers
        the query owns (worlds(), centres()).  bundles_per_world > 0: world = f
        // bundles_per_world, the shape of a world view's slab.  packed: a box
        per lane instead of a chunk of a bundle per group of 32 lanes (same
        words).  Simulator.close() frees what is left open."""
        return self._make(BoxQuery, "box queries need", bundles, boxes_per_bundle, max_hits,
                          world, centre, bundles_per_world, count, packed)

    def contact_query(self, max_contacts: int, select=None, poses: str = "solver",
                      plain: bool = False) -> "ContactQuery":
        """A ContactQuery: per world up to `max_contacts` touching primitive
        pairs of its rigid bodies with their manifolds (HIP backend, a simulator
        with a rigid-body step).  poses: "solver" (XPBD: where the last substep
        solved them) or "current".  select: None (every world), True (an owned
        int32 per world, selects()), a device tensor whose rows are the records
        or (ptr, record_bytes, first_byte).  plain: the generic routine, pair
        after pair (same words).  Simulator.close() frees what is left open."""
        return self._make(ContactQuery, "contact queries need", max_contacts, select, poses,
                          plain)

    def shape_query(self, bundles: int, shapes_per_bundle: int, max_hits: int, num_objects: int,
                    world=None, bundles_per_world: int = 0, count=None, exclude=None,
                    plain: bool = False) -> "ShapeQuery":
        """A ShapeQuery: `bundles` x `shapes_per_bundle` posed collision shapes
        tested against the rigid bodies of their worlds, up to `max_hits` hits
        each with their manifolds (HIP backend, a simulator with a rigid-body
        step).  num_objects: how many objects the simulator's ObjectManager
        holds.  world, exclude: None (owned buffers, worlds() / excludes()), a
        device tensor whose rows are the records or (ptr, record_bytes,
        first_byte); bundles_per_world > 0: world = f // bundles_per_world, and
        count (an int32 per world) skips the bundles at or past it.  plain: the
        generic routine, pair after pair (same words).  Simulator.close() frees
        what is left open."""
        return self._make(ShapeQuery, "shape queries need", bundles, shapes_per_bundle, max_hits,
                          num_objects, world, bundles_per_world, count, exclude, plain)

    def record(self, names: List[str], steps: int, on_render: bool = False) -> "Trajectory":
        """Records the exported tensors `names` on the device from the next
        replay on, `steps` slots each (see Trajectory): every replay of the
        step graph -- step(), step_async(), packed graphs -- or, with
        on_render, of the render graph.  HIP backend; raises on the reference
        backend, which has no executor to ask."""
        return self._make(Trajectory, "recording on the device needs", names, steps, on_render)

    # ---- stream-ordered stepping (HIP backend) -----------------------------------
    def stream(self) -> int:
        """hipStream_t of the executor's private stream (mwhip_stream)."""
        return int(runtime_lib().mwhip_stream(self.hip_exec()) or 0)

    def _pack_descriptor(self, names: List[str]):
        n = len(names)
        ptrs = (C.c_void_p * n)(*[self.tensor_ptr(name) for name in names])
        words = (C.c_uint32 * n)()
        for i, name in enumerate(names):
            _, dtype, dims, _ = self._tensor_info[name]
            if np.dtype(dtype).itemsize != 4:
                raise TypeError(f"{name}: only 4-byte element types are packed")
            words[i] = int(np.prod(dims[1:])) if len(dims) > 1 else 1
        return n, ptrs, words

    def packed_step_graph(self, names: List[str], dst_ptr: int) -> int:
        """A copy of the step graph whose last node packs the exported tensors
        `names` into one [worlds, words] int32 record per world at device
        address `dst_ptr` (mwhip_build_launch_graph_with_pack); replay it with
        step_async(graph=...)."""
        rt = runtime_lib()
        n, ptrs, words = self._pack_descriptor(names)
        out = C.c_uint64(0)
        self._check(rt.mwhip_build_launch_graph_with_pack(
            self.hip_exec(), self.lib.sim_hip_step_graph(self.handle), n, ptrs,
            words, self.num_worlds, dst_ptr, C.byref(out)), "mwhip_build_launch_graph_with_pack")
        return int(out.value)

    def step_async(self, n: int = 1, graph: int = 0) -> None:
        """Queues n replays of the step graph on the executor's stream without
        waiting for them (MWCudaExecutor::runAsync, reference mw_gpu.hpp:146):
        work that consumes the exported tensors must be ordered after this
        stream (events / sync()), as with any stream-ordered producer."""
        if self._async is None:     # (looked up once: this is a per-step call)
            rt = runtime_lib()
            exec_ = self.hip_exec()
            self._async = (rt, exec_, self.lib.sim_hip_step_graph(self.handle),
                           rt.mwhip_stream(exec_))
        rt, exec_, step_graph, stream = self._async
        graph = graph or step_graph
        for _ in range(n):
            rc = rt.mwhip_run_async(exec_, graph, stream)
            if rc != 0:
                self._check(rc, "mwhip_run_async")

    def set_input_ring(self, name: str, ring_ptr: int, num_slots: int) -> None:
        """The k-th replay after this call starts by copying slot k % num_slots
        of the device-resident ring at `ring_ptr` (num_slots x the tensor's
        bytes) into exported tensor `name` (mwhip_set_input_ring); ring_ptr = 0
        removes the ring."""
        rt = runtime_lib()
        _, dtype, dims, _ = self._tensor_info[name]
        slot_bytes = int(np.prod(dims)) * dtype.itemsize
        self._check(rt.mwhip_set_input_ring(self.hip_exec(), self.tensor_ptr(name),
                                            ring_ptr or None, slot_bytes, num_slots),
                    "mwhip_set_input_ring")

    def stream_wait_replays(self, hip_stream: int) -> None:
        """Makes `hip_stream` (a hipStream_t) wait for every replay queued so
        far, without putting anything on the executor's stream
        (mwhip_stream_wait_replays)."""
        rt = runtime_lib() if self._async is None else self._async[0]
        self._check(rt.mwhip_stream_wait_replays(self.hip_exec(), hip_stream),
                    "mwhip_stream_wait_replays")

    def pack_rows_async(self, names: List[str], dst_ptr: int) -> None:
        """Queues, behind the replays queued so far, the packing of the exported
        tensors `names` into one [worlds, words] int32 record per world at
        device address `dst_ptr` (mwhip_pack_rows)."""
        rt = runtime_lib()
        n, ptrs, words = self._pack_descriptor(names)
        self._check(rt.mwhip_pack_rows(self.hip_exec(), n, ptrs, words,
                                       self.num_worlds, dst_ptr), "mwhip_pack_rows")

    def sync(self) -> None:
        """Waits for the queued replays; raises on a device-side error flag."""
        self._check(runtime_lib().mwhip_synchronize(self.hip_exec()), "mwhip_synchronize")

    def profile(self, reps: int = 20, graph: int = 0):
        """Per-kernel timing of one step (HIP events on the executor's stream,
        kernels queued back to back behind a gate).  Advances the simulation by
        `reps` steps.  graph: another launch graph of this executor (e.g.
        render_graph()) instead of the step graph.  Returns a list of dicts."""
        rt = runtime_lib()
        stats = (KernelStat * 512)()
        n = rt.mwhip_profile(self.hip_exec(),
                             graph or self.lib.sim_hip_step_graph(self.handle),
                             reps, stats, 512)
        if n < 0:
            self._check(n, "mwhip_profile")
        return [dict(name=stats[i].name.decode(), kind=int(stats[i].node_kind),
                     avg_us=float(stats[i].avg_us), algo_bytes=float(stats[i].algo_bytes),
                     rows=float(stats[i].rows),
                     io_declared=bool(stats[i].io_declared),
                     workgroups=int(stats[i].workgroups),
                     node_index=int(stats[i].node_index)) for i in range(n)]
