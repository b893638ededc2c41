"""Time of a world write apply (mwhip_write_apply_async) at the BASELINE
configs[2] shape -- escape_room_phys, 8192 worlds, after 50 steps: the
rigid-body table's Position, Rotation and Velocity, max_rows = the largest
world's row count, take = max_rows, the slabs holding a view of the same
columns (so the state is the same for every repetition) -- next to two
yardsticks that are not this project's kernel:
  (a) the apply;
  (b) ONE contiguous device-to-device hipMemcpyAsync of the bytes (a) writes
      (the listed cells of the table's rows): a sorted table without holes is
      a block copy per world, so this is the floor;
  (c) the torch route a user has without world writes: worldOffsets and
      worldCounts read back from the device, indices built from them, one
      indexed assignment per column from the padded tensor.
Every figure is the median of REPS repetitions, each timed with a pair of HIP
events on the executor's own stream around the calls named, after WARM untimed
repetitions of the same call; between repetitions the stream is idle.
Then the cost of ONE step write in the step graph at the same shape (the shape
of bench.py's headline): the write launch's own time from mwhip_profile next
to the sum of every other launch of the same profiled steps, which are the
launches the step has without a step write.  Writes profiles/write_times.md:
    python profiles/tools/write_time.py [worlds] [out.md]"""
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
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "write_times.md")
SIM, TABLE, STEPS, DENOM, SEED = "escape_room_phys", "PhysicsEntity", 50, 200, 5
COLUMNS = ["PhysicsEntity.Position", "PhysicsEntity.Rotation", "PhysicsEntity.Velocity"]
REPS, WARM, PROFILE_REPS = 20, 3, 10
VIEW_OVER_FLOOR = 1.39      # profiles/view_times.md, the same shape
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
        raise SystemExit("write_time.py measures on the GPU; none is visible")
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
        with sim.world_view(TABLE, COLUMNS, max_rows=max_rows) as view, \
                sim.world_write(TABLE, COLUMNS, max_rows=max_rows) as write:
            cells = [write.cell_bytes(n) for n in COLUMNS]
            written_bytes = rows * sum(cells)
            read_bytes = rows * (sum(cells) + 4) + W * 4
            view.compute()
            before = [view.tensor(n).cpu().numpy() for n in COLUMNS]
            for name in COLUMNS:
                write.tensor(name).copy_(view.tensor(name))
            write.take.fill_(max_rows)
            torch.cuda.synchronize()
            results.append(("(a) write apply", timed(stream, write.apply_async)))
            write.apply()
            assert np.array_equal(write.counts.cpu().numpy(), per_world), \
                "the write's counts are not the dump's"
            view.compute()
            for name, was in zip(COLUMNS, before):
                assert np.array_equal(view.tensor(name).cpu().numpy(), was), \
                    "writing a view back changed " + name

            src, dst = C.c_void_p(), C.c_void_p()
            hip_check(hip.hipMalloc(C.byref(src), written_bytes), "hipMalloc")
            hip_check(hip.hipMalloc(C.byref(dst), written_bytes), "hipMalloc")
            results.append((
                "(b) one contiguous hipMemcpyAsync of the bytes (a) writes",
                timed(stream, lambda: hip_check(
                    hip.hipMemcpyAsync(dst, src, written_bytes, D2D, stream),
                    "hipMemcpyAsync"))))

            # (c): the columns as torch tensors, the work on the executor's stream
            device = torch.device("cuda", sim.gpu_id)
            ext = torch.cuda.ExternalStream(stream.value, device=device)
            col_index = {hdr.columnComponent[c]: c for c in range(hdr.numColumns)}
            cols, slabs = [], []
            for name, cell in zip(COLUMNS, cells):
                base = hdr.columns[col_index[column_ids(sim, name)[1]]]
                cols.append(torch.as_tensor(DeviceColumn(base, np.float32, (rows, cell // 4)),
                                            device=device))
                slabs.append(write.tensor(name, np.float32))
            offs_host = np.zeros(W, np.int32)
            cnts_host = np.zeros(W, np.int32)
            arange = torch.arange(max_rows, device=device, dtype=torch.int64)

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
                    index = (offs[:, None] + arange[None, :])[mask]
                    for col, slab in zip(cols, slabs):
                        col[index] = slab[mask]

            results.append(("(c) torch: offsets and counts read back, indexed assignment "
                            "per column", timed(stream, torch_route)))
            sim.sync()
            view.compute()
            for name, was in zip(COLUMNS, before):
                assert np.array_equal(view.tensor(name).cpu().numpy(), was), \
                    "the torch route and the write disagree on " + name
            hip.hipFree(src)
            hip.hipFree(dst)

            # one step write in the step graph: the launch's own time
            write.every_step()
            stats = sim.profile(PROFILE_REPS)
            at = [k["name"] for k in stats].index("write:write")
            assert at == 0, [k["name"] for k in stats][:3]
            step_write_us = stats[at]["avg_us"]
            step_write_bytes = stats[at]["algo_bytes"]
            rest_us = sum(k["avg_us"] for i, k in enumerate(stats) if i != at)
            launches = len(stats) - 1
            write.every_step(False)

    device_name = (f"{torch.cuda.get_device_name(0)} "
                   f"({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})")
    write_us, floor_us, torch_us = (r[1][0] for r in results)
    over_floor = write_us / floor_us
    if over_floor <= VIEW_OVER_FLOOR * 1.25:
        compare = (f"The view stands at {VIEW_OVER_FLOOR:.2f}x its floor at this shape "
                   "(profiles/view_times.md): the write is in the same place, as the same "
                   "walk in the other direction should be.")
    else:
        compare = (f"The view stands at {VIEW_OVER_FLOOR:.2f}x its floor at this shape "
                   "(profiles/view_times.md); the write is further from its own.  Its floor "
                   f"is smaller -- (b) moves {written_bytes} bytes, the view's floor the "
                   "WorldID cells too -- while the kernel still reads every WorldID cell, "
                   "take and the padded slabs' rows and pays the same launch and per-team "
                   "header reads, which do not shrink with the bytes.")
    if torch_us > write_us:
        against_torch = f"(a) against the torch route (c): {torch_us / write_us:.2f}x faster."
    else:
        against_torch = (f"(a) is NOT faster than the torch route (c): {write_us:.1f} us "
                         f"against {torch_us:.1f} us.")
    lines = [
        "# World writes: apply times",
        "",
        f"Written by `profiles/tools/write_time.py` on: {device_name}.",
        "",
        f"Shape of (a)-(c): `{SIM}`, {W} worlds, seed {SEED}, auto-reset 1/{DENOM}, after "
        f"{STEPS} steps (BASELINE configs[2]); table `{TABLE}` ({rows} rows, world-sorted, no "
        f"holes), columns Position, Rotation, Velocity ({sum(cells)} bytes per row), "
        f"max_rows = {max_rows} (the largest world's count), take = max_rows, the slabs "
        "holding a view of the same columns.",
        f"(a) writes {written_bytes} bytes (the listed cells of every row) and reads "
        f"{read_bytes} bytes (the same cells from the slabs, the WorldID cells and take).",
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
    lines += [
        "",
        f"(a) against the floor (b): {over_floor:.2f}x its time.  {against_torch}  "
        "Reported, not gated.",
        compare,
        "",
        "## One step write in the step graph",
        "",
        f"The same simulator and shape (the shape of `bench.py`'s headline), the write above "
        f"set as a step write, `mwhip_profile` over {PROFILE_REPS} steps: the launch "
        f"`write:write` takes {step_write_us:.1f} us of its own (algo_bytes "
        f"{step_write_bytes:.0f}); the other {launches} launches of the same steps, which are "
        f"the step as it is without a step write, take {rest_us:.1f} us together: "
        f"{100.0 * step_write_us / rest_us:.2f} % on top.  Kernel times between HIP events, "
        "not the step's wall time; with no step write set the launch does not exist.",
        "",
    ]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
