"""Time of a state digest (mwhip_digest_compute_async) at the BASELINE configs[2]
shape -- escape_room_phys, 8192 worlds, after 50 steps -- next to the other ways
of looking at all of the state, in the same process:
  (a) one compute_async over the full dump list (memset + kernel);
  (b) one snapshot save (mwhip_snapshot_save_async: prologue + copy kernel);
  (c) dump_all(): every column copied to the host, grouped by world;
  (d) windows of 200 queued replays of the step graph with and without
      every_step().
Every figure is the median of REPS timings, each with a pair of HIP events on
the executor's own stream around the calls named, after WARM untimed
repetitions, with the stream idle before each.  (c) is host work between the
two events, so its window is wall time seen from the stream.  The expectation
reported against: (a) does not exceed (b) -- the digest reads a subset of the
bytes the save reads and writes almost nothing.  Writes profiles/digest_times.md:
    python profiles/tools/digest_time.py [worlds] [out.md]"""
import ctypes as C
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from madrona_amd.simlib import Simulator, hip_lib_path

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "digest_times.md")
SIM, STEPS, DENOM, SEED = "escape_room_phys", 50, 200, 5
REPS, WARM, WINDOW = 20, 3, 200


def hip_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> hipError {rc}")


def main():
    import torch    # (its HIP runtime is the one every library of the process binds to)
    if not torch.cuda.is_available():
        raise SystemExit("digest_time.py measures on the GPU; none is visible")
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]

    with Simulator(hip_lib_path(SIM), W, seed=SEED, flags=DENOM) as sim:
        sim.step(STEPS)
        stream = C.c_void_p(sim.stream())
        dig = sim.digest()
        snap = sim.snapshot()
        snap.save()
        ev0, ev1 = C.c_void_p(), C.c_void_p()
        hip_check(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
        hip_check(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

        def timed(fn, reps=REPS, warm=WARM):
            times = []
            for rep in range(warm + reps):
                hip_check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
                hip_check(hip.hipEventRecord(ev0, stream), "hipEventRecord")
                fn()
                hip_check(hip.hipEventRecord(ev1, stream), "hipEventRecord")
                hip_check(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
                ms = C.c_float(0)
                hip_check(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1),
                          "hipEventElapsedTime")
                if rep >= warm:
                    times.append(ms.value * 1e3)
            return statistics.median(times), min(times), max(times)

        dump = sim.dump_all()
        cell_bytes = sum(rows.nbytes for rows, _ in dump.values())
        results = [
            ("(a) compute_async, full dump list", timed(dig.compute_async)),
            ("(b) snapshot save_async", timed(snap.save_async)),
            ("(c) dump_all()", timed(sim.dump_all, reps=5, warm=1)),
        ]
        snap_bytes = snap.nbytes
        # (the windows advance the simulation: the same number of steps for both)
        without = timed(lambda: sim.step_async(WINDOW), reps=REPS, warm=1)
        dig.every_step()
        with_digest = timed(lambda: sim.step_async(WINDOW), reps=REPS, warm=1)
        dig.every_step(False)
        sim.sync()
        results += [
            (f"(d) {WINDOW} queued replays, no step digest", without),
            (f"(d) {WINDOW} queued replays, every_step()", with_digest),
        ]
        groups = list(dig.groups)
        snap.close()
        dig.close()

    device = (f"{torch.cuda.get_device_name(0)} "
              f"({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})")
    a, b = results[0][1], results[1][1]
    spread_b = b[2] - b[1]
    lines = [
        "# State digest: times",
        "",
        f"Written by `profiles/tools/digest_time.py` on: {device}.",
        "",
        f"Shape: `{SIM}`, {W} worlds, seed {SEED}, auto-reset 1/{DENOM}, after {STEPS} steps "
        "(BASELINE configs[2]).",
        f"The full dump list: {len(dump)} columns in {len(groups)} tables, {cell_bytes} bytes of "
        f"cells ({cell_bytes / 2**20:.1f} MiB); the snapshot holds {snap_bytes} bytes "
        f"({snap_bytes / 2**20:.1f} MiB).",
        "",
        f"Median of {REPS} (min - max) after {WARM} untimed repetitions ((c): 5 after 1; "
        "(d): after 1), each timed with two HIP events on the executor's stream around the "
        "calls named, with the stream idle before it.",
        "",
        "| what | median us | min - max us |",
        "|---|---:|---:|",
    ]
    for name, (med, lo, hi) in results:
        lines.append(f"| {name} | {med:.1f} | {lo:.1f} - {hi:.1f} |")
    per_step = (with_digest[0] - without[0]) / WINDOW
    lines += [
        "",
        f"(a) reads {cell_bytes / a[0] / 1e3:.1f} GB/s of cells.  "
        f"every_step() adds {per_step:.2f} us per queued replay "
        f"({without[0] / WINDOW:.1f} -> {with_digest[0] / WINDOW:.1f} us).",
        "",
    ]
    if a[0] <= b[0]:
        lines.append(f"Expectation met: (a) {a[0]:.1f} us does not exceed (b) {b[0]:.1f} us.")
    elif a[0] - b[0] <= spread_b:
        lines.append(f"(a) {a[0]:.1f} us exceeds (b) {b[0]:.1f} us by less than (b)'s own "
                     f"run-to-run spread ({spread_b:.1f} us).")
    else:
        lines.append(f"EXPECTATION MISSED: (a) {a[0]:.1f} us exceeds (b) {b[0]:.1f} us by more "
                     f"than (b)'s own run-to-run spread ({spread_b:.1f} us).  The wide cells "
                     "(one lane walks a whole cell: lanes of a wavefront read addresses a "
                     "cell apart) are the first place to look.")
    lines.append("")
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
