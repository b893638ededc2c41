"""Time of a world reduce compute (mwhip_reduce_compute_async) at the BASELINE
configs[2] shape -- escape_room_phys, 8192 worlds, after 50 steps: ABSMAX,
COUNT_NONFINITE and SUM of the rigid-body table's Position, Rotation and
Velocity -- next to two yardsticks that are not this project's kernel:
  (a) the reduce compute;
  (b) ONE contiguous device-to-device hipMemcpyAsync of the bytes (a) reads
      (the listed cells and the WorldID cells of the table's rows): the floor;
  (c) the route there was before: a world view compute of the same columns
      (max_rows = the largest world's row count) and the torch reductions over
      its padded tensors that give tensors of the same shapes and types;
  (d) the general path: sort_stress, 8192 worlds, six ops of Item.Vec3, right
      after its ChurnOnly task graph (holes in the sorted prefix, new rows
      behind it: every team scans the tail).
Every figure is the median of REPS repetitions, each timed with a pair of HIP
events on the executor's own stream around the calls named, after WARM untimed
repetitions of the same call.  The state is the same for all of them; between
repetitions the stream is idle.  Writes profiles/reduce_times.md:
    python profiles/tools/reduce_time.py [worlds] [out.md]"""
import ctypes as C
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "reduce_times.md")
SIM, TABLE, STEPS, DENOM, SEED = "escape_room_phys", "PhysicsEntity", 50, 200, 5
COLUMNS = ["PhysicsEntity.Position", "PhysicsEntity.Rotation", "PhysicsEntity.Velocity"]
OPS = ["absmax", "count_nonfinite", "sum"]
STRESS_STEPS, CHURN_ONLY = 10, 1
REPS, WARM = 20, 3
D2D, D2H = 3, 2     # hipMemcpyDeviceToDevice, hipMemcpyDeviceToHost


def hip_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> hipError {rc}")


def main():
    import torch    # (its HIP runtime is the one every library of the process binds to)
    if not torch.cuda.is_available():
        raise SystemExit("reduce_time.py measures on the GPU; none is visible")
    runtime_lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]

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

    results = []
    terms = [(name, op) for name in COLUMNS for op in OPS]
    with Simulator(hip_lib_path(SIM), W, seed=SEED, flags=DENOM) as sim:
        sim.step(STEPS)
        stream = C.c_void_p(sim.stream())
        names = [c[0] for c in sim.columns]
        _, per_world = sim.dump_column(names.index(COLUMNS[0]), 512)
        max_rows, rows = int(per_world.max()), int(per_world.sum())
        with sim.world_reduce(TABLE, terms) as reduce, \
                sim.world_view(TABLE, COLUMNS, max_rows=max_rows) as view:
            cells = [view.cell_bytes(n) for n in COLUMNS]
            elems = sum(t.elems for _, t in reduce.terms)
            read_bytes = rows * (sum(cells) + 4)
            written_bytes = W * (4 * elems + 8)
            results.append(("(a) reduce compute", timed(stream, reduce.compute_async)))
            reduce.compute()
            assert np.array_equal(reduce.counts.cpu().numpy(), per_world), \
                "the reduce's counts are not the dump's"

            src, dst = C.c_void_p(), C.c_void_p()
            hip_check(hip.hipMalloc(C.byref(src), read_bytes), "hipMalloc")
            hip_check(hip.hipMalloc(C.byref(dst), read_bytes), "hipMalloc")
            results.append((
                "(b) one contiguous hipMemcpyAsync of the bytes (a) reads",
                timed(stream, lambda: hip_check(
                    hip.hipMemcpyAsync(dst, src, read_bytes, D2D, stream), "hipMemcpyAsync"))))

            # (c): the view, then torch over its padded tensors, on the executor's stream
            device = torch.device("cuda", sim.gpu_id)
            ext = torch.cuda.ExternalStream(stream.value, device=device)
            padded = [view.tensor(name, np.float32) for name in COLUMNS]
            keep = []

            def view_route():
                view.compute_async()
                with torch.cuda.stream(ext):
                    out = []
                    for x in padded:
                        out.append(torch.nan_to_num(x.abs(), nan=0.0, posinf=float("inf"))
                                   .amax(1))
                        out.append((~torch.isfinite(x)).sum(1, dtype=torch.int32))
                        out.append(x.sum(1))
                    keep[:] = out

            results.append(("(c) a view compute of the same columns and the torch reductions "
                            "over its tensors", timed(stream, view_route)))
            view_only = timed(stream, view.compute_async)
            sim.sync()
            sum_gap = 0.0
            for i, (_, term) in enumerate(reduce.terms):
                got, other = reduce.tensor(i).cpu().numpy(), keep[i].cpu().numpy()
                assert got.shape == other.shape and got.dtype == other.dtype, (i, term)
                if term.op == "sum":
                    # (torch adds in another order: close, not equal)
                    sum_gap = max(sum_gap, float(np.abs(got - other).max()))
                else:
                    assert np.array_equal(got.view(np.uint32), other.view(np.uint32)), \
                        ("the view route and the reduce disagree", i, term)
            hip.hipFree(src)
            hip.hipFree(dst)

    stress_terms = [("Item.Vec3", op) for op in
                    ("sum", "min", "max", "absmax", "count_nonzero", "count_nonfinite")]
    with Simulator(hip_lib_path("sort_stress"), W, seed=7) as sim:
        sim.step(STRESS_STEPS)
        sim.run_taskgraph(CHURN_ONLY)
        stream = C.c_void_p(sim.stream())
        names = [c[0] for c in sim.columns]
        world = sim.dump_column_raw(names.index("Item.WorldID"), 1 << 20).view(np.int32).ravel()
        stress_rows, stress_dead = len(world), int((world < 0).sum())
        with sim.world_reduce("Item", stress_terms) as reduce:
            stress = timed(stream, reduce.compute_async)
            sim.sync()
            stress_live = int(reduce.counts.cpu().numpy().sum())
            assert stress_live == stress_rows - stress_dead

    device_name = (f"{torch.cuda.get_device_name(0)} "
                   f"({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})")
    reduce_us, floor_us, route_us = (r[1][0] for r in results)
    lines = [
        "# World reduces: compute times",
        "",
        f"Written by `profiles/tools/reduce_time.py` on: {device_name}.",
        "",
        f"Shape of (a)-(c): `{SIM}`, {W} worlds, seed {SEED}, auto-reset 1/{DENOM}, after "
        f"{STEPS} steps (BASELINE configs[2]); table `{TABLE}` ({rows} rows, world-sorted, no "
        f"holes, at most {max_rows} per world), ABSMAX, COUNT_NONFINITE and SUM of Position, "
        f"Rotation and Velocity: {len(terms)} terms, {elems} elements, {sum(cells)} bytes per row.",
        f"(a) reads {read_bytes} bytes (the listed cells and the WorldID cells) and writes "
        f"{written_bytes} bytes (the results, the counts and the alarms).",
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
    lines.append(f"| (the view compute of (c) alone) | {view_only[0]:.1f} | "
                 f"{view_only[1]:.1f} - {view_only[2]:.1f} |")
    lines.append(f"| (d) general path: `sort_stress`, {W} worlds, after {STRESS_STEPS} steps and "
                 f"ChurnOnly | {stress[0]:.1f} | {stress[1]:.1f} - {stress[2]:.1f} |")
    lines += [
        "",
        f"(a) against the floor (b): {reduce_us / floor_us:.2f}x its time.  "
        f"(a) against the route through a view (c): {route_us / reduce_us:.2f}x faster.  "
        "Reported, not gated.",
        "(c) gives the same ABSMAX and COUNT_NONFINITE tensors bit for bit; its sums are "
        f"torch's, added in another order (largest difference here: {sum_gap:.3g}).",
        f"(d): table `Item`, {stress_rows} rows of which {stress_dead} are destroyed in place; "
        f"the six ops of Vec3 (18 elements, 32 lanes per world, two worlds per wavefront).  "
        "Every team scans the WorldID cells of the rows behind the sorted prefix.",
        "",
    ]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
