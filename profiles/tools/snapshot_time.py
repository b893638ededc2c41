"""Time of an executor snapshot (mwhip_snapshot_save_async / _restore_async) at
the BASELINE configs[2] shape -- escape_room_phys, 8192 worlds, after 50 steps --
next to two yardsticks that are the HIP runtime's, not this project's:
  (a) ONE contiguous device-to-device hipMemcpyAsync of the same byte count:
      the floor;
  (b) one hipMemcpyAsync per segment, with the segment lengths (row counts)
      and current column addresses read back from the device first: what a
      caller would do without the kernel.
Every figure is the median of REPS repetitions, each timed with a pair of HIP
events on the executor's own stream around the calls named (so a window holds
the launches' gaps too: for a save, the one-workgroup prologue, the gap, and
the copy kernel; for (b), the read-back's round trip and every copy), after
WARM untimed repetitions of the same call.  The state is the same for all of
them; between repetitions the stream is idle.  Writes profiles/snapshot_times.md:
    python profiles/tools/snapshot_time.py [worlds] [out.md]"""
import ctypes as C
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles",
                                                         "snapshot_times.md")
SIM, STEPS, DENOM, SEED = "escape_room_phys", 50, 200, 5
REPS, WARM = 20, 3
D2D = 3     # hipMemcpyDeviceToDevice


class Segment(C.Structure):
    _fields_ = [("live", C.c_void_p), ("saved", C.c_void_p), ("num_bytes", C.c_uint64)]


def hip_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> hipError {rc}")


def main():
    import torch    # (its HIP runtime is the one every library of the process binds to)
    if not torch.cuda.is_available():
        raise SystemExit("snapshot_time.py measures on the GPU; none is visible")
    rt = runtime_lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    rt.mwhip_snapshot_segments.restype = C.c_int32
    rt.mwhip_snapshot_segments.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(Segment),
                                           C.c_uint32]

    with Simulator(hip_lib_path(SIM), W, seed=SEED, flags=DENOM) as sim:
        sim.step(STEPS)
        stream = C.c_void_p(sim.stream())
        exec_ = sim.hip_exec()
        snap = sim.snapshot()
        snap.save()
        nbytes = snap.nbytes
        max_segments = 1 << 16
        segments = (Segment * max_segments)()

        def read_segments():
            n = rt.mwhip_snapshot_segments(exec_, snap.handle, segments, max_segments)
            if n < 0 or n > max_segments:
                raise RuntimeError(f"mwhip_snapshot_segments -> {n}")
            return n

        num_segments = read_segments()
        live_segments = sum(1 for i in range(num_segments) if segments[i].num_bytes)
        assert sum(segments[i].num_bytes for i in range(num_segments)) == nbytes

        ev0, ev1 = C.c_void_p(), C.c_void_p()
        hip_check(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
        hip_check(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

        def timed(fn):
            times = []
            for rep in range(WARM + REPS):
                hip_check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
                hip_check(hip.hipEventRecord(ev0, stream), "hipEventRecord")
                fn()
                hip_check(hip.hipEventRecord(ev1, stream), "hipEventRecord")
                hip_check(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
                ms = C.c_float(0)
                hip_check(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1),
                          "hipEventElapsedTime")
                if rep >= WARM:
                    times.append(ms.value * 1e3)
            return statistics.median(times), min(times), max(times)

        src, dst = C.c_void_p(), C.c_void_p()
        hip_check(hip.hipMalloc(C.byref(src), nbytes), "hipMalloc")
        hip_check(hip.hipMalloc(C.byref(dst), nbytes), "hipMalloc")

        def one_copy():
            hip_check(hip.hipMemcpyAsync(dst, src, nbytes, D2D, stream), "hipMemcpyAsync")

        def copy_per_segment():
            n = read_segments()     # waits, reads lengths and column addresses back
            for i in range(n):
                s = segments[i]
                if s.num_bytes:
                    hip_check(hip.hipMemcpyAsync(s.saved, s.live, s.num_bytes, D2D, stream),
                              "hipMemcpyAsync")

        results = [
            ("save (prologue + copy kernel)", timed(snap.save_async)),
            ("restore (copy kernel)", timed(snap.restore_async)),
            ("(a) one contiguous hipMemcpyAsync, device to device", timed(one_copy)),
            ("(b) lengths read back, then one hipMemcpyAsync per segment",
             timed(copy_per_segment)),
        ]
        sim.sync()
        hip.hipFree(src)
        hip.hipFree(dst)
        snap.close()

    # (the marketing name comes from a table that is not installed everywhere:
    # the architecture says which part it is)
    device = (f"{torch.cuda.get_device_name(0)} "
              f"({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})")
    save_us, floor_us, naive_us = results[0][1][0], results[2][1][0], results[3][1][0]
    lines = [
        "# Executor snapshot: save and restore times",
        "",
        f"Written by `profiles/tools/snapshot_time.py` on: {device}.",
        "",
        f"Shape: `{SIM}`, {W} worlds, seed {SEED}, auto-reset 1/{DENOM}, after {STEPS} steps "
        "(BASELINE configs[2]).",
        f"`mwhip_snapshot_bytes`: {nbytes} bytes ({nbytes / 2**20:.1f} MiB) in "
        f"{live_segments} non-empty segments of {num_segments}.",
        "",
        f"Median of {REPS} (min - max), after {WARM} untimed repetitions; each repetition "
        "is timed with two HIP events on the executor's stream around the calls named, "
        "with the stream idle before it.  GB/s = bytes copied / time "
        "(read and written once each).",
        "",
        "| what | median us | min - max us | GB/s |",
        "|---|---:|---:|---:|",
    ]
    for name, (med, lo, hi) in results:
        lines.append(f"| {name} | {med:.1f} | {lo:.1f} - {hi:.1f} | "
                     f"{nbytes / med / 1e3:.1f} |")
    lines += [
        "",
        f"Save against (b): {naive_us / save_us:.2f}x faster.  "
        f"Save against the floor (a): {save_us / floor_us:.2f}x its time "
        "(reported, not gated: many short segments do not reach a streaming copy's rate).",
        "",
    ]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
