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


def runtime_lib() -> C.CDLL:
    """libmadrona_hip.so (the C ABI of include/mwhip.h)."""
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
    lib.mwhip_snapshot_create.restype = C.c_int
    lib.mwhip_snapshot_create.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.mwhip_snapshot_destroy.restype = None
    lib.mwhip_snapshot_destroy.argtypes = [C.c_void_p, C.c_uint64]
    for fn in (lib.mwhip_snapshot_save, lib.mwhip_snapshot_restore,
               lib.mwhip_snapshot_save_async, lib.mwhip_snapshot_restore_async):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_snapshot_bytes.restype = C.c_uint64
    lib.mwhip_snapshot_bytes.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_digest_create.restype = C.c_int
    lib.mwhip_digest_create.argtypes = [C.c_void_p, C.POINTER(DigestColumn), C.c_uint32,
                                        C.POINTER(C.c_uint64)]
    lib.mwhip_digest_destroy.restype = None
    lib.mwhip_digest_destroy.argtypes = [C.c_void_p, C.c_uint64]
    for fn in (lib.mwhip_digest_compute, lib.mwhip_digest_compute_async,
               lib.mwhip_set_step_digest):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_digest_buffer.restype = C.c_void_p
    lib.mwhip_digest_buffer.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32)]
    lib.mwhip_digest_group.restype = C.c_int
    lib.mwhip_digest_group.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32,
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.mwhip_view_create.restype = C.c_int
    lib.mwhip_view_create.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32),
                                      C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.mwhip_view_destroy.restype = None
    lib.mwhip_view_destroy.argtypes = [C.c_void_p, C.c_uint64]
    for fn in (lib.mwhip_view_compute, lib.mwhip_view_compute_async):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_view_buffer.restype = C.c_void_p
    lib.mwhip_view_buffer.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.mwhip_view_counts.restype = C.c_void_p
    lib.mwhip_view_counts.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_set_step_view.restype = C.c_int
    lib.mwhip_set_step_view.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    lib.mwhip_write_create.restype = C.c_int
    lib.mwhip_write_create.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32),
                                       C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.mwhip_write_destroy.restype = None
    lib.mwhip_write_destroy.argtypes = [C.c_void_p, C.c_uint64]
    for fn in (lib.mwhip_write_apply, lib.mwhip_write_apply_async):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_write_buffer.restype = C.c_void_p
    lib.mwhip_write_buffer.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32,
                                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    for fn in (lib.mwhip_write_take, lib.mwhip_write_counts):
        fn.restype = C.c_void_p
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_set_step_write.restype = C.c_int
    lib.mwhip_set_step_write.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    lib.mwhip_reduce_create.restype = C.c_int
    lib.mwhip_reduce_create.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(ReduceTerm),
                                        C.c_uint32, C.POINTER(C.c_uint64)]
    lib.mwhip_reduce_destroy.restype = None
    lib.mwhip_reduce_destroy.argtypes = [C.c_void_p, C.c_uint64]
    for fn in (lib.mwhip_reduce_compute, lib.mwhip_reduce_compute_async):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_reduce_buffer.restype = C.c_void_p
    lib.mwhip_reduce_buffer.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32,
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    for fn in (lib.mwhip_reduce_counts, lib.mwhip_reduce_alarm):
        fn.restype = C.c_void_p
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_set_step_reduce.restype = C.c_int
    lib.mwhip_set_step_reduce.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    lib.mwhip_gather_create.restype = C.c_int
    lib.mwhip_gather_create.argtypes = [C.c_void_p, C.POINTER(GatherSource),
                                        C.POINTER(C.c_uint32), C.c_uint32,
                                        C.POINTER(C.c_uint64)]
    lib.mwhip_gather_destroy.restype = None
    lib.mwhip_gather_destroy.argtypes = [C.c_void_p, C.c_uint64]
    for fn in (lib.mwhip_gather_compute, lib.mwhip_gather_compute_async):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_gather_buffer.restype = C.c_void_p
    lib.mwhip_gather_buffer.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32,
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    for fn in (lib.mwhip_gather_archetypes, lib.mwhip_gather_worlds):
        fn.restype = C.c_void_p
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_set_step_gather.restype = C.c_int
    lib.mwhip_set_step_gather.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    lib.mwhip_scatter_create.restype = C.c_int
    lib.mwhip_scatter_create.argtypes = [C.c_void_p, C.POINTER(GatherSource),
                                         C.POINTER(C.c_uint32), C.c_uint32,
                                         C.POINTER(C.c_uint64)]
    lib.mwhip_scatter_destroy.restype = None
    lib.mwhip_scatter_destroy.argtypes = [C.c_void_p, C.c_uint64]
    for fn in (lib.mwhip_scatter_apply, lib.mwhip_scatter_apply_async):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_scatter_buffer.restype = C.c_void_p
    lib.mwhip_scatter_buffer.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    for fn in (lib.mwhip_scatter_select, lib.mwhip_scatter_archetypes,
               lib.mwhip_scatter_worlds, lib.mwhip_scatter_written):
        fn.restype = C.c_void_p
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_set_step_scatter.restype = C.c_int
    lib.mwhip_set_step_scatter.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    lib.mwhip_rays_create.restype = C.c_int
    lib.mwhip_rays_create.argtypes = [C.c_void_p, C.POINTER(RaysDesc), C.POINTER(C.c_uint64)]
    lib.mwhip_rays_destroy.restype = None
    lib.mwhip_rays_destroy.argtypes = [C.c_void_p, C.c_uint64]
    for fn in (lib.mwhip_rays_compute, lib.mwhip_rays_compute_async):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_rays_buffer.restype = C.c_void_p
    lib.mwhip_rays_buffer.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.mwhip_set_step_rays.restype = C.c_int
    lib.mwhip_set_step_rays.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    lib.mwhip_set_ray_kernel.restype = C.c_int
    lib.mwhip_set_ray_kernel.argtypes = [C.c_void_p, C.c_void_p]
    lib.mwhip_boxes_create.restype = C.c_int
    lib.mwhip_boxes_create.argtypes = [C.c_void_p, C.POINTER(BoxesDesc), C.POINTER(C.c_uint64)]
    lib.mwhip_boxes_destroy.restype = None
    lib.mwhip_boxes_destroy.argtypes = [C.c_void_p, C.c_uint64]
    for fn in (lib.mwhip_boxes_compute, lib.mwhip_boxes_compute_async):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint64]
    lib.mwhip_boxes_buffer.restype = C.c_void_p
    lib.mwhip_boxes_buffer.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.mwhip_set_step_boxes.restype = C.c_int
    lib.mwhip_set_step_boxes.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    lib.mwhip_set_box_kernel.restype = C.c_int
    lib.mwhip_set_box_kernel.argtypes = [C.c_void_p, C.c_void_p]
    return lib


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
    """What Snapshot, StateDigest, WorldView, WorldWrite, WorldReduce, EntityGather, EntityScatter, RayQuery and BoxQuery are: something a simulator's
    executor owns, named by `handle` there, kept in one of the simulator's
    lists (`_list`) while it is open.  close() frees it and takes it off the
    list (a snapshot too, which used to stay on it until the simulator closed); Simulator.close() frees the executor and orphans
    what is left: close() then does nothing, anything else raises."""

    _kind = "object"    # in messages
    _destroy = ""       # the runtime's destroy call
    _list = ""          # the simulator's list of the open ones
    _sim = None
    _exec = 0
    handle = 0

    def _live(self) -> int:
        # (the executor pointer dies with the simulator: never passed on then)
        if self._sim is None:
            raise RuntimeError(f"this {self._kind} is closed (or its simulator is)")
        return self.handle

    def _orphan(self) -> None:
        """Simulator.close(): the executor has freed (or is about to free) it."""
        self.handle = 0
        self._exec = 0
        self._sim = None

    def close(self) -> None:
        if self._sim is not None:
            if self.handle:
                getattr(self._rt, self._destroy)(self._exec, self.handle)
            open_ones = getattr(self._sim, self._list)
            if self in open_ones:
                open_ones.remove(self)
        self._orphan()


class Snapshot(_ExecObject):
    """One saved copy of all world state of a HIP-backend simulator, in device
    memory (mwhip_snapshot_*, include/mwhip.h): save() / restore() wait,
    save_async() / restore_async() are queued on the executor's stream behind
    the replays queued so far (step_async).  Reusable; belongs to the
    simulator that made it; Simulator.close() frees what is left and empties
    those snapshots (their close() then does nothing, any other call raises).
    Not rewound: the executor's replay count (the input
    ring's slot position) and the rgb / depth outputs of the render pass."""

    _kind, _destroy, _list = "snapshot", "mwhip_snapshot_destroy", "_snapshots"

    def __init__(self, sim: "Simulator"):
        self._rt = runtime_lib()
        self._exec = sim.hip_exec()
        if not self._exec:
            raise RuntimeError("snapshots need the HIP backend")
        handle = C.c_uint64(0)
        self._check(self._rt.mwhip_snapshot_create(self._exec, C.byref(handle)),
                    "mwhip_snapshot_create")
        self.handle = int(handle.value)
        self._sim = sim

    def save(self) -> None:
        self._check(self._rt.mwhip_snapshot_save(self._exec, self._live()),
                    "mwhip_snapshot_save")

    def restore(self) -> None:
        self._check(self._rt.mwhip_snapshot_restore(self._exec, self._live()),
                    "mwhip_snapshot_restore")

    def save_async(self) -> None:
        self._check(self._rt.mwhip_snapshot_save_async(self._exec, self._live()),
                    "mwhip_snapshot_save_async")

    def restore_async(self) -> None:
        self._check(self._rt.mwhip_snapshot_restore_async(self._exec, self._live()),
                    "mwhip_snapshot_restore_async")

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


class StateDigest(_ExecObject):
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

    _kind, _destroy, _list = "digest", "mwhip_digest_destroy", "_digests"

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
        self._sim = sim
        self._tables = [names[i].split(".", 1)[0] for i in self._indices]
        self.num_worlds = sim.num_worlds
        self.handle = 0
        self._exec = 0
        self._rt = None
        self._tensor = None
        self._every_step = False
        if sim.backend != "hip":
            self.groups = [key for key, _, _ in digest_ref.plan_groups(self._tables)]
            return
        if not hasattr(sim.lib, "sim_hip_column_ids"):
            raise RuntimeError("this simulator library has no sim_hip_column_ids: rebuild it")
        self._rt = runtime_lib()
        self._exec = sim.hip_exec()
        plan = (DigestColumn * len(self._indices))()
        for p, idx in enumerate(self._indices):
            arch, comp = C.c_uint32(0), C.c_uint32(0)
            if sim.lib.sim_hip_column_ids(sim.handle, idx, C.byref(arch), C.byref(comp)) != 0:
                raise RuntimeError(f"sim_hip_column_ids({idx}) failed")
            plan[p] = DigestColumn(arch.value, comp.value)
        handle = C.c_uint64(0)
        self._check(self._rt.mwhip_digest_create(self._exec, plan, len(self._indices),
                                                 C.byref(handle)), "mwhip_digest_create")
        self.handle = int(handle.value)
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

    def _orphan(self) -> None:
        super()._orphan()
        self._tensor = None

    def compute(self) -> np.ndarray:
        """uint64 [groups, worlds]; waits for the executor's stream."""
        if self._rt is None:
            super()._live()
            sim = self._sim
            return digest_ref.digest_of_dump(
                self._tables, [sim.dump_column(i) for i in self._indices], self.num_worlds)
        self._check(self._rt.mwhip_digest_compute(self._exec, self._live()),
                    "mwhip_digest_compute")
        return self.read()

    def read(self) -> np.ndarray:
        """The device buffer as it is (what the last compute, compute_async or
        step left), uint64 [groups, worlds]; waits for the executor's stream."""
        self._live()
        self._sim.sync()
        return self.tensor.cpu().numpy().view(np.uint64)

    def compute_async(self) -> None:
        handle = self._live()
        self._check(self._rt.mwhip_digest_compute_async(self._exec, handle),
                    "mwhip_digest_compute_async")

    @property
    def tensor(self):
        """torch int64 [groups, worlds] over the device buffer (no copy)."""
        self._live()
        if self._tensor is None:
            import torch

            from .tensor import DeviceColumn
            self._tensor = torch.as_tensor(
                DeviceColumn(self.buffer_ptr, np.int64, (len(self.groups), self.num_worlds)),
                device=torch.device("cuda", self._sim.gpu_id))
        return self._tensor

    def every_step(self, on: bool = True) -> None:
        """Every replay of a step graph recomputes this digest (waits for the
        stream and rebuilds the launch graphs); on=False turns it off again."""
        handle = self._live()
        if not on and not self._every_step:
            return
        self._check(self._rt.mwhip_set_step_digest(self._exec, handle if on else 0),
                    "mwhip_set_step_digest")
        self._every_step = bool(on)
        # (the rebuilt graphs are looked up by the same handles)


class WorldView(_ExecObject):
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

    _kind, _destroy, _list = "world view", "mwhip_view_destroy", "_views"

    def __init__(self, sim: "Simulator", table: str, columns, max_rows: int):
        names = [c[0] for c in sim._columns]
        of_table = [n for n in names if n.split(".", 1)[0] == table]
        if not of_table:
            raise KeyError(f"world_view(): no table {table!r} in the dump list")
        if columns is None:
            columns = of_table
        columns = list(columns)
        for name in columns:
            if name not in of_table:
                raise KeyError(f"world_view(): {name!r} is not a column of table {table!r}")
        if not columns:
            raise ValueError("world_view(): no columns")
        if len(set(columns)) != len(columns):
            raise ValueError("world_view(): a column is listed twice")
        if not hasattr(sim.lib, "sim_hip_column_ids"):
            raise RuntimeError("this simulator library has no sim_hip_column_ids: rebuild it")
        self._sim = sim
        self.table = table
        self.columns = columns
        self.max_rows = int(max_rows)
        self.num_worlds = sim.num_worlds
        self._rt = runtime_lib()
        self._exec = sim.hip_exec()
        self._tensors = {}
        self._every_step = False
        self.handle = 0
        archetypes = set()
        comps = (C.c_uint32 * len(columns))()
        for p, name in enumerate(columns):
            arch, comp = C.c_uint32(0), C.c_uint32(0)
            if sim.lib.sim_hip_column_ids(sim.handle, names.index(name), C.byref(arch),
                                          C.byref(comp)) != 0:
                raise RuntimeError(f"sim_hip_column_ids({name}) failed")
            archetypes.add(arch.value)
            comps[p] = comp.value
        assert len(archetypes) == 1, archetypes
        self.archetype = archetypes.pop()
        handle = C.c_uint64(0)
        self._check(self._rt.mwhip_view_create(
            self._exec, self.archetype, comps, len(columns),
            min(max(self.max_rows, 0), 0xFFFFFFFF), C.byref(handle)), "mwhip_view_create")
        self.handle = int(handle.value)
        self._buffers = {}
        for p, name in enumerate(columns):
            nbytes, cell = C.c_uint64(0), C.c_uint32(0)
            ptr = self._rt.mwhip_view_buffer(self._exec, self.handle, p, C.byref(nbytes),
                                             C.byref(cell))
            assert ptr and nbytes.value == self.num_worlds * self.max_rows * cell.value
            self._buffers[name] = (int(ptr), int(cell.value))
        self.counts_ptr = int(self._rt.mwhip_view_counts(self._exec, self.handle) or 0)

    def _orphan(self) -> None:
        super()._orphan()
        self._tensors = {}

    def compute(self) -> "WorldView":
        """Rewrites every buffer and the counts; waits for the executor's stream."""
        self._check(self._rt.mwhip_view_compute(self._exec, self._live()),
                    "mwhip_view_compute")
        return self

    def compute_async(self) -> None:
        self._check(self._rt.mwhip_view_compute_async(self._exec, self._live()),
                    "mwhip_view_compute_async")

    def buffer_ptr(self, name: str) -> int:
        """Device address of column `name`'s [worlds, max_rows, cell_bytes] bytes."""
        self._live()
        return self._buffers[name][0]

    def cell_bytes(self, name: str) -> int:
        return self._buffers[name][1]

    def _wrap(self, key, ptr, dtype, shape):
        if key not in self._tensors:
            import torch

            from .tensor import DeviceColumn
            self._tensors[key] = torch.as_tensor(
                DeviceColumn(ptr, dtype, shape),
                device=torch.device("cuda", self._sim.gpu_id))
        return self._tensors[key]

    def tensor(self, name: str, dtype=None):
        """torch uint8 [worlds, max_rows, cell_bytes] over the device buffer of
        column `name` (no copy), or, with a numpy dtype, [worlds, max_rows,
        cell_bytes // itemsize] of that type."""
        self._live()
        ptr, cell = self._buffers[name]
        dt = np.dtype(np.uint8 if dtype is None else dtype)
        if cell % dt.itemsize != 0:
            raise TypeError(f"{name}: cells of {cell} bytes do not hold whole {dt} items")
        return self._wrap((name, dt.str), ptr, dt.type,
                          (self.num_worlds, self.max_rows, cell // dt.itemsize))

    @property
    def counts(self):
        """torch int32 [worlds] over the device buffer (no copy): each world's
        rows in the table, which may exceed max_rows."""
        self._live()
        return self._wrap(("", "counts"), self.counts_ptr, np.int32, (self.num_worlds,))

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

    def every_step(self, on: bool = True) -> None:
        """Every replay of a step graph recomputes this view (waits for the
        stream and rebuilds the launch graphs); on=False turns it off again."""
        handle = self._live()
        if not on and not self._every_step:
            return
        self._check(self._rt.mwhip_set_step_view(self._exec, handle, 1 if on else 0),
                    "mwhip_set_step_view")
        self._every_step = bool(on)


class WorldWrite(_ExecObject):
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

    _kind, _destroy, _list = "world write", "mwhip_write_destroy", "_writes"

    def __init__(self, sim: "Simulator", table: str, columns, max_rows: int):
        names = [c[0] for c in sim._columns]
        of_table = [n for n in names if n.split(".", 1)[0] == table]
        if not of_table:
            raise KeyError(f"world_write(): no table {table!r} in the dump list")
        if not hasattr(sim.lib, "sim_hip_column_ids"):
            raise RuntimeError("this simulator library has no sim_hip_column_ids: rebuild it")

        def ids(name):
            arch, comp = C.c_uint32(0), C.c_uint32(0)
            if sim.lib.sim_hip_column_ids(sim.handle, names.index(name), C.byref(arch),
                                          C.byref(comp)) != 0:
                raise RuntimeError(f"sim_hip_column_ids({name}) failed")
            return arch.value, comp.value

        if columns is None:
            # (component 0 is Entity, 1 is WorldID: include/mwhip.h)
            columns = [n for n in of_table if ids(n)[1] not in (0, 1)]
        columns = list(columns)
        for name in columns:
            if name not in of_table:
                raise KeyError(f"world_write(): {name!r} is not a column of table {table!r}")
        if not columns:
            raise ValueError("world_write(): no columns")
        if len(set(columns)) != len(columns):
            raise ValueError("world_write(): a column is listed twice")
        self._sim = sim
        self.table = table
        self.columns = columns
        self.max_rows = int(max_rows)
        self.num_worlds = sim.num_worlds
        self._rt = runtime_lib()
        self._exec = sim.hip_exec()
        self._tensors = {}
        self._every_step = False
        self.handle = 0
        archetypes = set()
        comps = (C.c_uint32 * len(columns))()
        for p, name in enumerate(columns):
            arch, comps[p] = ids(name)
            archetypes.add(arch)
        assert len(archetypes) == 1, archetypes
        self.archetype = archetypes.pop()
        handle = C.c_uint64(0)
        self._check(self._rt.mwhip_write_create(
            self._exec, self.archetype, comps, len(columns),
            min(max(self.max_rows, 0), 0xFFFFFFFF), C.byref(handle)), "mwhip_write_create")
        self.handle = int(handle.value)
        self._buffers = {}
        for p, name in enumerate(columns):
            nbytes, cell = C.c_uint64(0), C.c_uint32(0)
            ptr = self._rt.mwhip_write_buffer(self._exec, self.handle, p, C.byref(nbytes),
                                              C.byref(cell))
            assert ptr and nbytes.value == self.num_worlds * self.max_rows * cell.value
            self._buffers[name] = (int(ptr), int(cell.value))
        self._take_ptr = int(self._rt.mwhip_write_take(self._exec, self.handle) or 0)
        self.counts_ptr = int(self._rt.mwhip_write_counts(self._exec, self.handle) or 0)

    def _orphan(self) -> None:
        super()._orphan()
        self._tensors = {}

    def apply(self) -> "WorldWrite":
        """Writes the table; waits for the executor's stream."""
        self._check(self._rt.mwhip_write_apply(self._exec, self._live()),
                    "mwhip_write_apply")
        return self

    def apply_async(self) -> None:
        self._check(self._rt.mwhip_write_apply_async(self._exec, self._live()),
                    "mwhip_write_apply_async")

    def buffer_ptr(self, name: str) -> int:
        """Device address of column `name`'s [worlds, max_rows, cell_bytes] bytes."""
        self._live()
        return self._buffers[name][0]

    def cell_bytes(self, name: str) -> int:
        return self._buffers[name][1]

    @property
    def take_ptr(self) -> int:
        """Device address of the int32 [worlds] take buffer."""
        self._live()
        return self._take_ptr

    _wrap = WorldView._wrap

    def tensor(self, name: str, dtype=None):
        """torch uint8 [worlds, max_rows, cell_bytes] over the device buffer of
        column `name` (no copy), or, with a numpy dtype, [worlds, max_rows,
        cell_bytes // itemsize] of that type.  The caller fills it."""
        self._live()
        ptr, cell = self._buffers[name]
        dt = np.dtype(np.uint8 if dtype is None else dtype)
        if cell % dt.itemsize != 0:
            raise TypeError(f"{name}: cells of {cell} bytes do not hold whole {dt} items")
        return self._wrap((name, dt.str), ptr, dt.type,
                          (self.num_worlds, self.max_rows, cell // dt.itemsize))

    @property
    def take(self):
        """torch int32 [worlds] over the device buffer (no copy): the leading
        rows of each world to write.  The caller fills it."""
        self._live()
        return self._wrap(("", "take"), self._take_ptr, np.int32, (self.num_worlds,))

    @property
    def counts(self):
        """torch int32 [worlds] over the device buffer (no copy): each world's
        rows in the table as the last apply found them, not clipped."""
        self._live()
        return self._wrap(("", "counts"), self.counts_ptr, np.int32, (self.num_worlds,))

    def every_step(self, on: bool = True) -> None:
        """Every replay of a step graph applies this write first (waits for the
        stream and rebuilds the launch graphs); on=False turns it off again."""
        handle = self._live()
        if not on and not self._every_step:
            return
        self._check(self._rt.mwhip_set_step_write(self._exec, handle, 1 if on else 0),
                    "mwhip_set_step_write")
        self._every_step = bool(on)


class WorldReduce(_ExecObject):
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

    _kind, _destroy, _list = "world reduce", "mwhip_reduce_destroy", "_reduces"

    def __init__(self, sim: "Simulator", table: str, terms):
        from . import reduce_ref

        info = {c[0]: c for c in sim._columns}
        names = list(info)
        of_table = [n for n in names if n.split(".", 1)[0] == table]
        if not of_table:
            raise KeyError(f"world_reduce(): no table {table!r} in the dump list")
        if not hasattr(sim.lib, "sim_hip_column_ids"):
            raise RuntimeError("this simulator library has no sim_hip_column_ids: rebuild it")
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
        self._sim = sim
        self.table = table
        self.num_worlds = sim.num_worlds
        self._rt = runtime_lib()
        self._exec = sim.hip_exec()
        self._tensors = {}
        self._every_step = False
        self.handle = 0
        archetypes = set()
        arr = (ReduceTerm * len(self.terms))()
        for p, (column, term) in enumerate(self.terms):
            arch, comp = C.c_uint32(0), C.c_uint32(0)
            if sim.lib.sim_hip_column_ids(sim.handle, names.index(column), C.byref(arch),
                                          C.byref(comp)) != 0:
                raise RuntimeError(f"sim_hip_column_ids({column}) failed")
            archetypes.add(arch.value)
            arr[p] = ReduceTerm(comp.value, min(max(term.offset, 0), 0xFFFFFFFF),
                                min(max(term.elems, 0), 0xFFFFFFFF),
                                reduce_ref.DTYPES[term.dtype], reduce_ref.OPS[term.op],
                                reduce_ref.ALARM if term.alarm else 0, term.limit)
        assert len(archetypes) == 1, archetypes
        self.archetype = archetypes.pop()
        handle = C.c_uint64(0)
        self._check(self._rt.mwhip_reduce_create(self._exec, self.archetype, arr, len(self.terms),
                                                 C.byref(handle)), "mwhip_reduce_create")
        self.handle = int(handle.value)
        self._buffers = []
        for p, (_, term) in enumerate(self.terms):
            nbytes, elems = C.c_uint64(0), C.c_uint32(0)
            ptr = self._rt.mwhip_reduce_buffer(self._exec, self.handle, p, C.byref(nbytes),
                                               C.byref(elems))
            assert ptr and elems.value == term.elems and \
                nbytes.value == self.num_worlds * term.elems * 4
            self._buffers.append((int(ptr), reduce_ref.result_dtype(term)))
        self.counts_ptr = int(self._rt.mwhip_reduce_counts(self._exec, self.handle) or 0)
        self._alarm_ptr = int(self._rt.mwhip_reduce_alarm(self._exec, self.handle) or 0)

    def _orphan(self) -> None:
        super()._orphan()
        self._tensors = {}

    def compute(self) -> "WorldReduce":
        """Rewrites every buffer; waits for the executor's stream."""
        self._check(self._rt.mwhip_reduce_compute(self._exec, self._live()),
                    "mwhip_reduce_compute")
        return self

    def compute_async(self) -> None:
        self._check(self._rt.mwhip_reduce_compute_async(self._exec, self._live()),
                    "mwhip_reduce_compute_async")

    def buffer_ptr(self, i: int) -> int:
        """Device address of term i's [worlds, elems] results (4 bytes each)."""
        self._live()
        return self._buffers[i][0]

    @property
    def alarm_ptr(self) -> int:
        """Device address of the int32 [worlds] alarm buffer."""
        self._live()
        return self._alarm_ptr

    _wrap = WorldView._wrap

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
        self._live()
        return self._wrap(("", "counts"), self.counts_ptr, np.int32, (self.num_worlds,))

    @property
    def alarm(self):
        """torch int32 [worlds] over the device buffer (no copy): 1 where an
        alarm term tripped in the last compute, else 0."""
        self._live()
        return self._wrap(("", "alarm"), self._alarm_ptr, np.int32, (self.num_worlds,))

    def every_step(self, on: bool = True) -> None:
        """Every replay of a step graph recomputes this reduce (waits for the
        stream and rebuilds the launch graphs); on=False turns it off again."""
        handle = self._live()
        if not on and not self._every_step:
            return
        self._check(self._rt.mwhip_set_step_reduce(self._exec, handle, 1 if on else 0),
                    "mwhip_set_step_reduce")
        self._every_step = bool(on)


class _HandleCells(_ExecObject):
    """What EntityGather and EntityScatter share: a source of N handles, a list
    of components named as the dump list names them, per component a device
    buffer of N cells, and int32 [N] archetypes and worlds."""

    _what = "entity_gather()"   # in messages

    @classmethod
    def _component_list(cls, sim: "Simulator", components):
        """(the component ids as a C array, the names as a list)"""
        if not hasattr(sim.lib, "sim_hip_column_ids"):
            raise RuntimeError("this simulator library has no sim_hip_column_ids: rebuild it")
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
            arch, comp = C.c_uint32(0), C.c_uint32(0)
            if sim.lib.sim_hip_column_ids(sim.handle, idx, C.byref(arch), C.byref(comp)) != 0:
                raise RuntimeError(f"sim_hip_column_ids({column[0]}) failed")
            ids.add(int(comp.value))
        if not ids:
            raise KeyError(f"{cls._what}: no column of the dump list is named "
                           f"'<table>.{name}'")
        if len(ids) != 1:
            raise KeyError(f"{cls._what}: {name!r} names different components "
                           f"{sorted(ids)} in different tables")
        return ids.pop()

    def _orphan(self) -> None:
        super()._orphan()
        self._tensors = {}
        self._source = None

    def buffer_ptr(self, name: str) -> int:
        """Device address of component `name`'s [N, cell_bytes] bytes."""
        self._live()
        return self._buffers[name][0]

    def cell_bytes(self, name: str) -> int:
        return self._buffers[name][1]

    _wrap = WorldView._wrap

    def tensor(self, name: str, dtype=None):
        """torch uint8 [N, cell_bytes] over the device buffer of component
        `name` (no copy), or, with a numpy dtype, [N, cell_bytes // itemsize]
        of that type."""
        self._live()
        ptr, cell = self._buffers[name]
        dt = np.dtype(np.uint8 if dtype is None else dtype)
        if cell % dt.itemsize != 0:
            raise TypeError(f"{name}: cells of {cell} bytes do not hold whole {dt} items")
        return self._wrap((name, dt.str), ptr, dt.type,
                          (self.num_handles, cell // dt.itemsize))

    @property
    def archetypes(self):
        """torch int32 [N] over the device buffer (no copy): the archetype of
        the entity each handle names, -1 where it names nothing."""
        self._live()
        return self._wrap(("", "archetypes"), self.archetypes_ptr, np.int32,
                          (self.num_handles,))

    @property
    def worlds(self):
        """torch int32 [N] over the device buffer (no copy): the world of the
        entity each handle names, -1 where it names nothing."""
        self._live()
        return self._wrap(("", "worlds"), self.worlds_ptr, np.int32, (self.num_handles,))


class EntityGather(_HandleCells):
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

    _kind, _destroy, _list = "entity gather", "mwhip_gather_destroy", "_gathers"

    def __init__(self, sim: "Simulator", source, components):
        comps, components = self._component_list(sim, components)
        # (a tensor stays where it is while the gather exists)
        self._source, ptr, num_records, record_bytes, first_byte, per = \
            self._handle_source(source)
        self._sim = sim
        self.components = components
        self.num_handles = num_records * per
        self._rt = runtime_lib()
        self._exec = sim.hip_exec()
        self._tensors = {}
        self._every_step = False
        self.handle = 0
        src = GatherSource(ptr, num_records, record_bytes, first_byte, per, 0)
        handle = C.c_uint64(0)
        self._check(self._rt.mwhip_gather_create(self._exec, C.byref(src), comps,
                                                 len(components), C.byref(handle)),
                    "mwhip_gather_create")
        self.handle = int(handle.value)
        self._buffers = {}
        for p, name in enumerate(components):
            nbytes, cell = C.c_uint64(0), C.c_uint32(0)
            buf = self._rt.mwhip_gather_buffer(self._exec, self.handle, p, C.byref(nbytes),
                                               C.byref(cell))
            assert buf and nbytes.value == self.num_handles * cell.value
            self._buffers[name] = (int(buf), int(cell.value))
        self.archetypes_ptr = int(self._rt.mwhip_gather_archetypes(self._exec, self.handle) or 0)
        self.worlds_ptr = int(self._rt.mwhip_gather_worlds(self._exec, self.handle) or 0)

    def compute(self) -> "EntityGather":
        """Rewrites every buffer, archetypes and worlds; waits for the
        executor's stream."""
        self._check(self._rt.mwhip_gather_compute(self._exec, self._live()),
                    "mwhip_gather_compute")
        return self

    def compute_async(self) -> None:
        self._check(self._rt.mwhip_gather_compute_async(self._exec, self._live()),
                    "mwhip_gather_compute_async")

    def every_step(self, on: bool = True) -> None:
        """Every replay of a step graph recomputes this gather (waits for the
        stream and rebuilds the launch graphs); on=False turns it off again."""
        handle = self._live()
        if not on and not self._every_step:
            return
        self._check(self._rt.mwhip_set_step_gather(self._exec, handle, 1 if on else 0),
                    "mwhip_set_step_gather")
        self._every_step = bool(on)


class EntityScatter(_HandleCells):
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

    _kind, _destroy, _list = "entity scatter", "mwhip_scatter_destroy", "_scatters"
    _what = "entity_scatter()"

    def __init__(self, sim: "Simulator", source, components):
        comps, components = self._component_list(sim, components)
        self._source, ptr, num_records, record_bytes, first_byte, per = \
            self._handle_source(source)
        self._sim = sim
        self.components = components
        self.num_handles = num_records * per
        self._rt = runtime_lib()
        self._exec = sim.hip_exec()
        self._tensors = {}
        self._every_step = False
        self.handle = 0
        src = GatherSource(ptr, num_records, record_bytes, first_byte, per, 0)
        handle = C.c_uint64(0)
        self._check(self._rt.mwhip_scatter_create(self._exec, C.byref(src), comps,
                                                  len(components), C.byref(handle)),
                    "mwhip_scatter_create")
        self.handle = int(handle.value)
        self._buffers = {}
        for p, name in enumerate(components):
            nbytes, cell = C.c_uint64(0), C.c_uint32(0)
            buf = self._rt.mwhip_scatter_buffer(self._exec, self.handle, p, C.byref(nbytes),
                                                C.byref(cell))
            assert buf and nbytes.value == self.num_handles * cell.value
            self._buffers[name] = (int(buf), int(cell.value))
        self.select_ptr = int(self._rt.mwhip_scatter_select(self._exec, self.handle) or 0)
        self.archetypes_ptr = int(self._rt.mwhip_scatter_archetypes(self._exec, self.handle) or 0)
        self.worlds_ptr = int(self._rt.mwhip_scatter_worlds(self._exec, self.handle) or 0)
        self.written_ptr = int(self._rt.mwhip_scatter_written(self._exec, self.handle) or 0)

    def apply(self) -> "EntityScatter":
        """Stores the selected cells and rewrites archetypes, worlds and
        written; waits for the executor's stream."""
        self._check(self._rt.mwhip_scatter_apply(self._exec, self._live()),
                    "mwhip_scatter_apply")
        return self

    def apply_async(self) -> None:
        self._check(self._rt.mwhip_scatter_apply_async(self._exec, self._live()),
                    "mwhip_scatter_apply_async")

    @property
    def select(self):
        """torch int32 [N] over the device buffer (no copy), the caller's to
        fill: handle i's cells are stored where it is non-zero."""
        self._live()
        return self._wrap(("", "select"), self.select_ptr, np.int32, (self.num_handles,))

    @property
    def written(self):
        """torch int32 [N] over the device buffer (no copy): 1 where the last
        apply stored handle i's cells (selected, names an entity, and no
        selected handle of higher index names the same one)."""
        self._live()
        return self._wrap(("", "written"), self.written_ptr, np.int32, (self.num_handles,))

    def every_step(self, on: bool = True) -> None:
        """Every replay of a step graph applies this scatter (waits for the
        stream and rebuilds the launch graphs); on=False turns it off again."""
        handle = self._live()
        if not on and not self._every_step:
            return
        self._check(self._rt.mwhip_set_step_scatter(self._exec, handle, 1 if on else 0),
                    "mwhip_set_step_scatter")
        self._every_step = bool(on)


class RayQuery(_ExecObject):
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

    _kind, _destroy, _list = "ray query", "mwhip_rays_destroy", "_ray_queries"
    HIT, MISS, SKIPPED, BAD_WORLD, BAD_RAY = 1, 0, -1, -2, -3
    _BUFS = {"world": 0, "origin": 1, "dir": 2, "t_max": 3, "hit_t": 4, "hit": 5, "normal": 6,
             "status": 7}

    @staticmethod
    def _source(what: str, source, item_bytes: int, who: str = "ray_query()"):
        """(the tensor to keep alive or None, RaySource) of None, a device
        tensor whose rows are the records, or (ptr, record_bytes, first_byte)"""
        if source is None:
            return None, RaySource(None, 0, 0)
        if isinstance(source, tuple):
            ptr, record_bytes, first_byte = (int(v) for v in source)
            return None, RaySource(ptr, record_bytes, first_byte)
        import torch

        if not isinstance(source, torch.Tensor) or not source.is_cuda:
            raise TypeError(f"{who}: {what} is a torch tensor on the device or a "
                            "(ptr, record_bytes, first_byte) tuple")
        if source.element_size() != 4 or not source.is_contiguous() or source.dim() < 1:
            raise TypeError(f"{who}: the {what} tensor must be contiguous with 4-byte "
                            f"items, not {source.dtype} {tuple(source.shape)}")
        record = item_bytes if source.dim() == 1 else int(source.shape[-1]) * 4
        if record < item_bytes:
            raise TypeError(f"{who}: rows of {record} bytes are too short for {what}")
        return source, RaySource(source.data_ptr(), record, 0)

    def __init__(self, sim: "Simulator", fans: int, rays_per_fan: int, world=None, origin=None,
                 fans_per_world: int = 0, count=None):
        self._sim = sim
        self.num_fans, self.rays_per_fan = int(fans), int(rays_per_fan)
        self.num_rays = self.num_fans * self.rays_per_fan
        self.fans_per_world = int(fans_per_world)
        self._rt = runtime_lib()
        self._exec = sim.hip_exec()
        self._tensors = {}
        self._every_step = False
        self.handle = 0
        desc = RaysDesc(self.num_fans, self.rays_per_fan, self.fans_per_world, 0)
        keep_w, desc.world = self._source("world", world, 4)
        keep_c, desc.count = self._source("count", count, 4)
        keep_o, desc.origin = self._source("origin", origin, 12)
        self._sources = (keep_w, keep_c, keep_o)    # (stay where they are)
        handle = C.c_uint64(0)
        self._check(self._rt.mwhip_rays_create(self._exec, C.byref(desc), C.byref(handle)),
                    "mwhip_rays_create")
        self.handle = int(handle.value)
        self._owned = {"world": world is None and self.fans_per_world == 0,
                       "origin": origin is None}

    def _orphan(self) -> None:
        super()._orphan()
        self._tensors = {}
        self._sources = ()

    _wrap = WorldView._wrap

    def buffer_ptr(self, name: str) -> int:
        """Device address of owned buffer `name`: world, origin, dir, t_max,
        hit_t, hit, normal or status."""
        handle = self._live()
        nbytes = C.c_uint64(0)
        ptr = self._rt.mwhip_rays_buffer(self._exec, handle, self._BUFS[name], C.byref(nbytes))
        if not ptr:
            raise RuntimeError(f"mwhip_rays_buffer({name}): "
                               f"{self._rt.mwhip_last_error().decode()}")
        return int(ptr)

    def _tensor(self, name, dtype, shape):
        self._live()
        if not self._owned.get(name, True):
            raise RuntimeError(f"this ray query owns no {name} buffer: " + (
                "fans_per_world gives each fan its world" if name == "world"
                and self.fans_per_world else f"a {name} source was given"))
        if name not in self._tensors:
            self._wrap(name, self.buffer_ptr(name), dtype, shape)
        return self._tensors[name]

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

    def compute(self) -> "RayQuery":
        """Rewrites every output; waits for the executor's stream."""
        self._check(self._rt.mwhip_rays_compute(self._exec, self._live()), "mwhip_rays_compute")
        return self

    def compute_async(self) -> None:
        self._check(self._rt.mwhip_rays_compute_async(self._exec, self._live()),
                    "mwhip_rays_compute_async")

    def every_step(self, on: bool = True) -> None:
        """Every replay of a step graph recomputes this query (waits for the
        stream and rebuilds the launch graphs); on=False turns it off again."""
        handle = self._live()
        if not on and not self._every_step:
            return
        self._check(self._rt.mwhip_set_step_rays(self._exec, handle, 1 if on else 0),
                    "mwhip_set_step_rays")
        self._every_step = bool(on)


class BoxQuery(_ExecObject):
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

    _kind, _destroy, _list = "box query", "mwhip_boxes_destroy", "_box_queries"
    OK, SKIPPED, BAD_WORLD, BAD_BOX = 0, -1, -2, -3
    PACKED = 1
    _BUFS = {"world": 0, "centre": 1, "lo": 2, "hi": 3, "status": 4, "count": 5, "hits": 6}

    def __init__(self, sim: "Simulator", bundles: int, boxes_per_bundle: int, max_hits: int,
                 world=None, centre=None, bundles_per_world: int = 0, count=None,
                 packed: bool = False):
        self._sim = sim
        self.num_bundles, self.boxes_per_bundle = int(bundles), int(boxes_per_bundle)
        self.max_hits = int(max_hits)
        self.num_boxes = self.num_bundles * self.boxes_per_bundle
        self.bundles_per_world = int(bundles_per_world)
        self.packed = bool(packed)
        self._rt = runtime_lib()
        self._exec = sim.hip_exec()
        self._tensors = {}
        self._every_step = False
        self.handle = 0
        desc = BoxesDesc(self.num_bundles, self.boxes_per_bundle, self.max_hits,
                         self.bundles_per_world, self.PACKED if self.packed else 0, 0)
        source = lambda what, src, nbytes: RayQuery._source(what, src, nbytes, "box_query()")
        keep_w, desc.world = source("world", world, 4)
        keep_c, desc.count = source("count", count, 4)
        keep_o, desc.centre = source("centre", centre, 12)
        self._sources = (keep_w, keep_c, keep_o)    # (stay where they are)
        handle = C.c_uint64(0)
        self._check(self._rt.mwhip_boxes_create(self._exec, C.byref(desc), C.byref(handle)),
                    "mwhip_boxes_create")
        self.handle = int(handle.value)
        self._owned = {"world": world is None and self.bundles_per_world == 0,
                       "centre": centre is None}

    def _orphan(self) -> None:
        super()._orphan()
        self._tensors = {}
        self._sources = ()

    _wrap = WorldView._wrap

    def buffer_ptr(self, name: str) -> int:
        """Device address of owned buffer `name`: world, centre, lo, hi, status,
        count or hits."""
        handle = self._live()
        nbytes = C.c_uint64(0)
        ptr = self._rt.mwhip_boxes_buffer(self._exec, handle, self._BUFS[name], C.byref(nbytes))
        if not ptr:
            raise RuntimeError(f"mwhip_boxes_buffer({name}): "
                               f"{self._rt.mwhip_last_error().decode()}")
        return int(ptr)

    def _tensor(self, name, dtype, shape):
        self._live()
        if not self._owned.get(name, True):
            raise RuntimeError(f"this box query owns no {name} buffer: " + (
                "bundles_per_world gives each bundle its world" if name == "world"
                and self.bundles_per_world else f"a {name} source was given"))
        if name not in self._tensors:
            self._wrap(name, self.buffer_ptr(name), dtype, shape)
        return self._tensors[name]

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

    def compute(self) -> "BoxQuery":
        """Rewrites every output; waits for the executor's stream."""
        self._check(self._rt.mwhip_boxes_compute(self._exec, self._live()),
                    "mwhip_boxes_compute")
        return self

    def compute_async(self) -> None:
        self._check(self._rt.mwhip_boxes_compute_async(self._exec, self._live()),
                    "mwhip_boxes_compute_async")

    def every_step(self, on: bool = True) -> None:
        """Every replay of a step graph recomputes this query (waits for the
        stream and rebuilds the launch graphs); on=False turns it off again."""
        handle = self._live()
        if not on and not self._every_step:
            return
        self._check(self._rt.mwhip_set_step_boxes(self._exec, handle, 1 if on else 0),
                    "mwhip_set_step_boxes")
        self._every_step = bool(on)


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
        self._snapshots: List["Snapshot"] = []
        self._trajectories: List["Trajectory"] = []
        self._digests: List["StateDigest"] = []
        self._views: List["WorldView"] = []
        self._writes: List["WorldWrite"] = []
        self._reduces: List["WorldReduce"] = []
        self._gathers: List["EntityGather"] = []
        self._scatters: List["EntityScatter"] = []
        self._ray_queries: List["RayQuery"] = []
        self._box_queries: List["BoxQuery"] = []
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
            # sim_destroy frees the executor and with it its snapshots, digests,
            # world views, world writes, world reduces, entity gathers,
            # entity scatters, ray queries and box queries, and
            # forgets its output rings (the trajectories keep their tensors)
            for open_ones in (self._snapshots, self._trajectories, self._digests, self._views,
                              self._writes, self._reduces, self._gathers, self._scatters,
                              self._ray_queries, self._box_queries):
                for obj in open_ones:
                    obj._orphan()
                open_ones.clear()
            self.lib.sim_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

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
        rc = self.lib.sim_hip_render(self.handle)
        if rc != 0:
            raise RuntimeError(f"sim_hip_render -> {rc}: "
                               f"{runtime_lib().mwhip_last_error().decode()}")

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

    def snapshot(self) -> "Snapshot":
        """A new, empty Snapshot of this simulator (HIP backend; raises on the
        reference backend, which has no executor to ask)."""
        if self.backend != "hip":
            raise RuntimeError(f"snapshots need the HIP backend, this is {self.backend!r}")
        snap = Snapshot(self)
        self._snapshots.append(snap)
        return snap

    def digest(self, columns=None) -> "StateDigest":
        """A StateDigest over `columns` of the dump list (names or indices, in
        that order; default: the whole dump list in its order).  Either
        backend: see StateDigest for what the reference backend offers."""
        dig = StateDigest(self, columns)
        self._digests.append(dig)
        return dig

    def world_view(self, table: str, columns=None, max_rows: int = 0) -> "WorldView":
        """A WorldView of `columns` (names as in `columns`, e.g. "Item.Vec3";
        default: every dump-list column of the table) of table `table`, padded
        to max_rows rows per world.  HIP backend; raises on the reference
        backend, which has no executor to ask."""
        if self.backend != "hip":
            raise RuntimeError(f"world views need the HIP backend, this is {self.backend!r}")
        view = WorldView(self, table, columns, max_rows)
        self._views.append(view)
        return view

    def world_write(self, table: str, columns=None, max_rows: int = 0) -> "WorldWrite":
        """A WorldWrite into `columns` (names as in `columns`, e.g. "Item.Vec3";
        default: every dump-list column of the table except Entity and
        WorldID, which cannot be written) of table `table`, max_rows rows per
        world.  HIP backend; raises on the reference backend, which has no
        executor to ask."""
        if self.backend != "hip":
            raise RuntimeError(f"world writes need the HIP backend, this is {self.backend!r}")
        write = WorldWrite(self, table, columns, max_rows)
        self._writes.append(write)
        return write

    def world_reduce(self, table: str, terms) -> "WorldReduce":
        """A WorldReduce of table `table`: one result per world and element for
        every term -- (column, op) or (column, op, options), see WorldReduce --
        plus each world's row count and an alarm word per world.  HIP backend;
        raises on the reference backend, which has no executor to ask."""
        if self.backend != "hip":
            raise RuntimeError(f"world reduces need the HIP backend, this is {self.backend!r}")
        reduce = WorldReduce(self, table, terms)
        self._reduces.append(reduce)
        return reduce

    def entity_gather(self, source, components) -> "EntityGather":
        """An EntityGather of `components` (named by the part of a dump-list
        column name behind the dot, e.g. "Position"; none: only archetypes and
        worlds) through the handles of `source`: a torch tensor on the device,
        contiguous, int32 / uint32 [..., 2] or uint8 [..., 8], or a (ptr,
        num_records, record_bytes, first_byte, handles_per_record) tuple such
        as WorldView.handle_source() gives.  HIP backend; raises on the
        reference backend, which has no executor to ask."""
        if self.backend != "hip":
            raise RuntimeError(f"entity gathers need the HIP backend, this is {self.backend!r}")
        gather = EntityGather(self, source, components)
        self._gathers.append(gather)
        return gather

    def entity_scatter(self, source, components) -> "EntityScatter":
        """An EntityScatter of `components` (named as entity_gather() names
        them; at least one, neither Entity nor WorldID) through the handles of
        `source`, which takes every form entity_gather() takes,
        WorldView.handle_source() included.  HIP backend; raises on the
        reference backend, which has no executor to ask."""
        if self.backend != "hip":
            raise RuntimeError(f"entity scatters need the HIP backend, this is {self.backend!r}")
        scatter = EntityScatter(self, source, components)
        self._scatters.append(scatter)
        return scatter

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
        if self.backend != "hip":
            raise RuntimeError(f"ray queries need the HIP backend, this is {self.backend!r}")
        query = RayQuery(self, fans, rays_per_fan, world, origin, fans_per_world, count)
        self._ray_queries.append(query)
        return query

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
        if self.backend != "hip":
            raise RuntimeError(f"box queries need the HIP backend, this is {self.backend!r}")
        query = BoxQuery(self, bundles, boxes_per_bundle, max_hits, world, centre,
                         bundles_per_world, count, packed)
        self._box_queries.append(query)
        return query

    def record(self, names: List[str], steps: int, on_render: bool = False) -> "Trajectory":
        """Records the exported tensors `names` on the device from the next
        replay on, `steps` slots each (see Trajectory): every replay of the
        step graph -- step(), step_async(), packed graphs -- or, with
        on_render, of the render graph.  HIP backend; raises on the reference
        backend, which has no executor to ask."""
        if self.backend != "hip":
            raise RuntimeError(
                f"recording on the device needs the HIP backend, this is {self.backend!r}")
        traj = Trajectory(self, names, steps, on_render)
        self._trajectories.append(traj)
        return traj

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
        rc = rt.mwhip_build_launch_graph_with_pack(
            self.hip_exec(), self.lib.sim_hip_step_graph(self.handle), n, ptrs,
            words, self.num_worlds, dst_ptr, C.byref(out))
        if rc != 0:
            raise RuntimeError(f"mwhip_build_launch_graph_with_pack -> {rc}: "
                               f"{rt.mwhip_last_error().decode()}")
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
                raise RuntimeError(
                    f"mwhip_run_async -> {rc}: {rt.mwhip_last_error().decode()}")

    def set_input_ring(self, name: str, ring_ptr: int, num_slots: int) -> None:
        """The k-th replay after this call starts by copying slot k % num_slots
        of the device-resident ring at `ring_ptr` (num_slots x the tensor's
        bytes) into exported tensor `name` (mwhip_set_input_ring); ring_ptr = 0
        removes the ring."""
        rt = runtime_lib()
        _, dtype, dims, _ = self._tensor_info[name]
        slot_bytes = int(np.prod(dims)) * dtype.itemsize
        rc = rt.mwhip_set_input_ring(self.hip_exec(), self.tensor_ptr(name),
                                     ring_ptr or None, slot_bytes, num_slots)
        if rc != 0:
            raise RuntimeError(f"mwhip_set_input_ring -> {rc}: "
                               f"{rt.mwhip_last_error().decode()}")

    def stream_wait_replays(self, hip_stream: int) -> None:
        """Makes `hip_stream` (a hipStream_t) wait for every replay queued so
        far, without putting anything on the executor's stream
        (mwhip_stream_wait_replays)."""
        rt = runtime_lib() if self._async is None else self._async[0]
        rc = rt.mwhip_stream_wait_replays(self.hip_exec(), hip_stream)
        if rc != 0:
            raise RuntimeError(f"mwhip_stream_wait_replays -> {rc}: "
                               f"{rt.mwhip_last_error().decode()}")

    def pack_rows_async(self, names: List[str], dst_ptr: int) -> None:
        """Queues, behind the replays queued so far, the packing of the exported
        tensors `names` into one [worlds, words] int32 record per world at
        device address `dst_ptr` (mwhip_pack_rows)."""
        rt = runtime_lib()
        n, ptrs, words = self._pack_descriptor(names)
        rc = rt.mwhip_pack_rows(self.hip_exec(), n, ptrs, words,
                                self.num_worlds, dst_ptr)
        if rc != 0:
            raise RuntimeError(
                f"mwhip_pack_rows -> {rc}: {rt.mwhip_last_error().decode()}")

    def sync(self) -> None:
        """Waits for the queued replays; raises on a device-side error flag."""
        rt = runtime_lib()
        rc = rt.mwhip_synchronize(self.hip_exec())
        if rc != 0:
            raise RuntimeError(
                f"mwhip_synchronize -> {rc}: {rt.mwhip_last_error().decode()}")

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
            raise RuntimeError(f"mwhip_profile -> {n}: {rt.mwhip_last_error().decode()}")
        return [dict(name=stats[i].name.decode(), kind=int(stats[i].node_kind),
                     avg_us=float(stats[i].avg_us), algo_bytes=float(stats[i].algo_bytes),
                     rows=float(stats[i].rows),
                     io_declared=bool(stats[i].io_declared),
                     workgroups=int(stats[i].workgroups),
                     node_index=int(stats[i].node_index)) for i in range(n)]
