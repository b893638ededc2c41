"""Time of a world view compute (mwhip_view_compute_async) at the BASELINE
configs[2] shape -- escape_room_phys, 8192 worlds, after 50 steps: the
rigid-body table's Position, Rotation and Velocity, max_rows = the largest
world's row count -- next to two yardsticks that are not this project's kernel:
  (a) the view compute;
  (b) ONE contiguous device-to-device hipMemcpyAsync of the bytes (a) reads
      (the listed cells and the WorldID cells of the table's rows): a sorted
      table without holes is a block copy per world, so this is the floor;
  (c) the torch route: worldOffsets and worldCounts read back from the device,
      indices built from them, one index_select per column into a padded
      tensor, the padding zeroed;
  (d) the general path: sort_stress, 8192 worlds, every Item column, right
      after its ChurnOnly task graph (holes in the sorted prefix, new rows
      behind it: every team scans the tail).
Every figure is the median of REPS repetitions, each timed with a pair of HIP
events on the executor's own stream around the calls named, after WARM untimed
repetitions of the same call.  The state is the same for all of them; between
repetitions the stream is idle.  Writes profiles/view_times.md:
    python profiles/tools/view_time.py [worlds] [out.md]"""
import ctypes as C
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib
from madrona_amd.tensor import DeviceColumn

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "view_times.md")
SIM, TABLE, STEPS, DENOM, SEED = "escape_room_phys", "PhysicsEntity", 50, 200, 5
COLUMNS = ["PhysicsEntity.Position", "PhysicsEntity.Rotation", "PhysicsEntity.Velocity"]
STRESS_STEPS, CHURN_ONLY = 10, 1
REPS, WARM = 20, 3
D2D, D2H = 3, 2     # hipMemcpyDeviceToDevice, hipMemcpyDeviceToHost
MAX_COLUMNS = 128   # kMaxColumns, include/madrona/mwhip/ecs_state.hpp


class TableHdr(C.Structure):
    """TableHdr (include/madrona/mwhip/ecs_state.hpp)"""
    _fields_ = [("columns", C.c_void_p * MAX_COLUMNS), ("columnsAlt", C.c_void_p * MAX_COLUMNS),
                ("columnBytes", C.c_uint32 * MAX_COLUMNS),
                ("columnFlags", C.c_uint32 * MAX_COLUMNS),
                ("columnComponent", C.c_uint16 * MAX_COLUMNS),
                ("numColumns", C.c_int32), ("numRows", C.c_int32), ("capacity", C.c_int32),
                ("needsSort", C.c_uint32), ("worldOffsets", C.c_void_p),
                ("worldCounts", C.c_void_p), ("maxPerWorld", C.c_uint32),
                ("registered", C.c_uint32), ("rowBytes", C.c_uint32), ("peakRows", C.c_int32),
                ("sortedRows", C.c_int32), ("tailRows", C.c_int32)]


def hip_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> hipError {rc}")


def main():
    import torch    # (its HIP runtime is the one every library of the process binds to)
    if not torch.cuda.is_available():
        raise SystemExit("view_time.py measures on the GPU; none is visible")
    rt = runtime_lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    rt.mwhip_table_header.restype = C.c_void_p
    rt.mwhip_table_header.argtypes = [C.c_void_p, C.c_uint32]

    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_check(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    hip_check(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    def timed(stream, fn):
        times = []
        for rep in range(WARM + REPS):
            hip_check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
            hip_check(hip.hipEventRecord(ev0, stream), "hipEventRecord")
            fn()
            hip_check(hip.hipEventRecord(ev1, stream), "hipEventRecord")
            hip_check(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
            ms = C.c_float(0)
            hip_check(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
            if rep >= WARM:
                times.append(ms.value * 1e3)
        return statistics.median(times), min(times), max(times)

    def header(sim, archetype):
        sim.sync()
        hdr = TableHdr()
        hip_check(hip.hipMemcpy(C.byref(hdr), rt.mwhip_table_header(sim.hip_exec(), archetype),
                                C.sizeof(hdr), D2H), "hipMemcpy")
        return hdr

    def column_ids(sim, name):
        arch, comp = C.c_uint32(0), C.c_uint32(0)
        names = [c[0] for c in sim.columns]
        assert sim.lib.sim_hip_column_ids(sim.handle, names.index(name), C.byref(arch),
                                          C.byref(comp)) == 0
        return arch.value, comp.value

    results = []
    with Simulator(hip_lib_path(SIM), W, seed=SEED, flags=DENOM) as sim:
        sim.step(STEPS)
        stream = C.c_void_p(sim.stream())
        names = [c[0] for c in sim.columns]
        _, per_world = sim.dump_column(names.index(COLUMNS[0]), 512)
        max_rows = int(per_world.max())
        archetype = column_ids(sim, COLUMNS[0])[0]
        hdr = header(sim, archetype)
        rows = hdr.numRows
        assert rows == int(per_world.sum()) and hdr.sortedRows == rows, \
            (rows, int(per_world.sum()), hdr.sortedRows)
        with sim.world_view(TABLE, COLUMNS, max_rows=max_rows) as view:
            cells = [view.cell_bytes(n) for n in COLUMNS]
            read_bytes = rows * (sum(cells) + 4)
            written_bytes = W * max_rows * sum(cells) + W * 4
            results.append(("(a) view compute", timed(stream, view.compute_async)))
            view.compute()
            counts = view.counts.cpu().numpy()
            assert np.array_equal(counts, per_world), "the view's counts are not the dump's"

            src, dst = C.c_void_p(), C.c_void_p()
            hip_check(hip.hipMalloc(C.byref(src), read_bytes), "hipMalloc")
            hip_check(hip.hipMalloc(C.byref(dst), read_bytes), "hipMalloc")
            results.append((
                "(b) one contiguous hipMemcpyAsync of the bytes (a) reads",
                timed(stream, lambda: hip_check(
                    hip.hipMemcpyAsync(dst, src, read_bytes, D2D, stream), "hipMemcpyAsync"))))

            # (c): the columns as torch tensors, the work on the executor's stream
            device = torch.device("cuda", sim.gpu_id)
            ext = torch.cuda.ExternalStream(stream.value, device=device)
            col_index = {hdr.columnComponent[c]: c for c in range(hdr.numColumns)}
            cols = []
            for name, cell in zip(COLUMNS, cells):
                base = hdr.columns[col_index[column_ids(sim, name)[1]]]
                cols.append(torch.as_tensor(DeviceColumn(base, np.float32, (rows, cell // 4)),
                                            device=device))
            offs_host = np.zeros(W, np.int32)
            cnts_host = np.zeros(W, np.int32)
            arange = torch.arange(max_rows, device=device, dtype=torch.int64)
            keep = []

            def torch_route():
                hip_check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
                hip_check(hip.hipMemcpy(offs_host.ctypes.data, hdr.worldOffsets, W * 4, D2H),
                          "hipMemcpy")
                hip_check(hip.hipMemcpy(cnts_host.ctypes.data, hdr.worldCounts, W * 4, D2H),
                          "hipMemcpy")
                with torch.cuda.stream(ext):
                    offs = torch.from_numpy(offs_host).to(device).to(torch.int64)
                    cnts = torch.from_numpy(cnts_host).to(device).to(torch.int64)
                    mask = arange[None, :] < cnts[:, None]
                    index = torch.where(mask, offs[:, None] + arange[None, :], 0).flatten()
                    keep[:] = [col.index_select(0, index).view(W, max_rows, -1) *
                               mask[:, :, None] for col in cols]

            results.append(("(c) torch: offsets and counts read back, index_select per column",
                            timed(stream, torch_route)))
            sim.sync()
            got = view.tensor(COLUMNS[0], np.float32).cpu().numpy()
            assert np.array_equal(keep[0].cpu().numpy().view(np.uint32), got.view(np.uint32)), \
                "the torch route and the view disagree"
            hip.hipFree(src)
            hip.hipFree(dst)

    with Simulator(hip_lib_path("sort_stress"), W, seed=7) as sim:
        sim.step(STRESS_STEPS)
        sim.run_taskgraph(CHURN_ONLY)
        stream = C.c_void_p(sim.stream())
        hdr = header(sim, column_ids(sim, "Item.Key")[0])
        stress_rows, stress_tail = hdr.numRows, hdr.numRows - hdr.sortedRows
        with sim.world_view("Item", max_rows=40) as view:
            stress_cells = sum(view.cell_bytes(n) for n in view.columns)
            stress = timed(stream, view.compute_async)
            sim.sync()
            stress_live = int(view.counts.cpu().numpy().sum())

    device_name = (f"{torch.cuda.get_device_name(0)} "
                   f"({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})")
    view_us, floor_us, torch_us = (r[1][0] for r in results)
    lines = [
        "# World views: compute times",
        "",
        f"Written by `profiles/tools/view_time.py` on: {device_name}.",
        "",
        f"Shape of (a)-(c): `{SIM}`, {W} worlds, seed {SEED}, auto-reset 1/{DENOM}, after "
        f"{STEPS} steps (BASELINE configs[2]); table `{TABLE}` ({rows} rows, world-sorted, no "
        f"holes), columns Position, Rotation, Velocity ({sum(cells)} bytes per row), "
        f"max_rows = {max_rows} (the largest world's count).",
        f"(a) reads {read_bytes} bytes (the listed cells and the WorldID cells) and writes "
        f"{written_bytes} bytes (the padded buffers and the counts).",
        "",
        f"Median of {REPS} (min - max), after {WARM} untimed repetitions; each repetition "
        "is timed with two HIP events on the executor's stream around the calls named, "
        "with the stream idle before it.",
        "",
        "| what | median us | min - max us |",
        "|---|---:|---:|",
    ]
    for name, (med, lo, hi) in results:
        lines.append(f"| {name} | {med:.1f} | {lo:.1f} - {hi:.1f} |")
    lines.append(f"| (d) general path: `sort_stress`, {W} worlds, after {STRESS_STEPS} steps and "
                 f"ChurnOnly | {stress[0]:.1f} | {stress[1]:.1f} - {stress[2]:.1f} |")
    lines += [
        "",
        f"(a) against the floor (b): {view_us / floor_us:.2f}x its time.  "
        f"(a) against the torch route (c): {torch_us / view_us:.2f}x faster.  "
        "Reported, not gated.",
        f"(d): table `Item`, {stress_rows} rows of which {stress_tail} sit behind the sorted "
        f"prefix and {stress_rows - stress_live} are destroyed in place; every Item column "
        f"({stress_cells} bytes per row), max_rows = 40.  Every team scans the "
        f"{stress_tail} WorldID cells of the tail.",
        "",
    ]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
