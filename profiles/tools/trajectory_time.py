"""What recording a rollout on the device costs (mwhip_set_output_ring,
Simulator.record) at the Hide-and-Seek observation set -- hideseek, 8192 worlds,
the seven tensors a trainer reads every step --, next to the
caller's only alternative without the rings:
  (a) the `ring.out` launch alone, from mwhip_profile, as GB/s next to the
      device copy rate of the same process (what bench.py reports as
      `hbm_measured`: a torch copy of 512 MiB, read + written);
  (b) a window of WINDOW step_async replays with the rings set;
  (c) the same window without rings;
  (d) the same window without rings but with one device-to-device
      hipMemcpyAsync per tensor per step on the executor's stream.
(b), (c), (d) are medians of REPS windows, each timed with a pair of HIP events
on the executor's stream with the stream idle before it, after WARM untimed
windows.  Reported, not gated.  Writes profiles/trajectory_times.md:
    python profiles/tools/trajectory_time.py [worlds] [out.md]"""
import ctypes as C
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from madrona_amd.simlib import Simulator, hip_lib_path

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles",
                                                         "trajectory_times.md")
SIM, SEED, FLAGS, SETTLE = "hideseek", 5, 40, 50
NAMES = ["self_obs", "agent_obs", "box_obs", "ramp_obs", "lidar", "reward", "done"]
WINDOW, REPS, WARM = 200, 5, 1
SLOTS = 8       # of every ring: 8 x 23.8 MB, rewritten round and round
D2D = 3         # hipMemcpyDeviceToDevice


def hip_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> hipError {rc}")


def copy_rate_gbps(torch):
    """bench.py's measure_hbm_bandwidth, the copy half: bytes moved per second."""
    n = 128 * 1024 * 1024
    a = torch.empty(n, dtype=torch.float32, device="cuda")
    b = torch.ones(n, dtype=torch.float32, device="cuda")
    for _ in range(3):
        a.copy_(b)
    torch.cuda.synchronize()
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(20):
        a.copy_(b)
    ev1.record()
    torch.cuda.synchronize()
    rate = 2 * 4 * n * 20 / (ev0.elapsed_time(ev1) * 1e-3) / 1e9
    del a, b
    torch.cuda.empty_cache()
    return rate


def main():
    import torch    # (its HIP runtime is the one every library of the process binds to)
    if not torch.cuda.is_available():
        raise SystemExit("trajectory_time.py measures on the GPU; none is visible")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]

    copy_gbps = copy_rate_gbps(torch)
    with Simulator(hip_lib_path(SIM), W, seed=SEED, flags=FLAGS) as sim:
        sim.step(SETTLE)
        stream = C.c_void_p(sim.stream())
        sizes = {}
        for name in NAMES:
            _, dtype, dims, _ = sim.tensor_meta(name)
            count = 1
            for d in dims:
                count *= d
            sizes[name] = count * dtype.itemsize
        step_bytes = sum(sizes.values())

        ev0, ev1 = C.c_void_p(), C.c_void_p()
        hip_check(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
        hip_check(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

        def window_us(one_step):
            times = []
            for rep in range(WARM + REPS):
                sim.sync()
                hip_check(hip.hipEventRecord(ev0, stream), "hipEventRecord")
                for k in range(WINDOW):
                    one_step(k)
                hip_check(hip.hipEventRecord(ev1, stream), "hipEventRecord")
                hip_check(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
                ms = C.c_float(0)
                hip_check(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1),
                          "hipEventElapsedTime")
                if rep >= WARM:
                    times.append(ms.value * 1e3 / WINDOW)
            sim.sync()
            return statistics.median(times), min(times), max(times)

        def plain_step(k):
            sim.step_async(1)

        # (c) no rings
        per_step_plain = window_us(plain_step)

        # (d) no rings, one hipMemcpyAsync per tensor per step
        buffers = {name: torch.empty(SLOTS * sizes[name], dtype=torch.uint8, device="cuda")
                   for name in NAMES}
        torch.cuda.synchronize()
        copies = [(buffers[name].data_ptr(), sim.tensor_ptr(name), sizes[name])
                  for name in NAMES]

        def step_and_copies(k):
            sim.step_async(1)
            slot = k % SLOTS
            for dst, src, size in copies:
                hip_check(hip.hipMemcpyAsync(dst + slot * size, src, size, D2D, stream),
                          "hipMemcpyAsync")

        per_step_copies = window_us(step_and_copies)
        del buffers

        # (b) the rings, and (a) their launch alone
        traj = sim.record(NAMES, SLOTS)
        per_step_rings = window_us(plain_step)
        ring_kernels = [k for k in sim.profile(reps=20) if "ring.out" in k["name"]]
        assert len(ring_kernels) == 1 and ring_kernels[0]["algo_bytes"] == 2 * step_bytes
        ring_us = ring_kernels[0]["avg_us"]
        ring_wgs = ring_kernels[0]["workgroups"]
        traj.close()

    device = (f"{torch.cuda.get_device_name(0)} "
              f"({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})")
    ring_gbps = 2 * step_bytes / ring_us / 1e3
    b_c = per_step_rings[0] - per_step_plain[0]
    d_c = per_step_copies[0] - per_step_plain[0]
    near = abs(b_c - ring_us) <= max(0.5 * ring_us, 5.0)
    under = b_c < 0.5 * d_c
    lines = [
        "# Recording a rollout on the device: what a step pays",
        "",
        f"Written by `profiles/tools/trajectory_time.py` on: {device}.",
        "",
        f"Shape: `{SIM}`, {W} worlds, seed {SEED}, flags {FLAGS}, after {SETTLE} steps; "
        f"tensors {', '.join(NAMES)}: {step_bytes} bytes ({step_bytes / 1e6:.1f} MB) per "
        f"step, rings of {SLOTS} slots.",
        "",
        f"(a) the `ring.out` launch alone (`mwhip_profile`, mean of 20, {ring_wgs} "
        f"workgroups): {ring_us:.1f} us = {ring_gbps:.0f} GB/s read + written; the device "
        f"copy rate of this process (torch copy of 512 MiB, bench.py's `hbm_measured`): "
        f"{copy_gbps:.0f} GB/s.",
        "",
        f"Windows of {WINDOW} `step_async` replays, us per step: median of {REPS} windows "
        f"(min - max) after {WARM} untimed; two HIP events on the executor's stream around "
        "each window, the stream idle before it.",
        "",
        "| what | median us / step | min - max |",
        "|---|---:|---:|",
    ]
    for name, (med, lo, hi) in (("(b) rings set", per_step_rings),
                                ("(c) no rings", per_step_plain),
                                ("(d) no rings, one hipMemcpyAsync per tensor per step",
                                 per_step_copies)):
        lines.append(f"| {name} | {med:.1f} | {lo:.1f} - {hi:.1f} |")
    lines += [
        "",
        f"(b - c) = {b_c:.1f} us per step; (d - c) = {d_c:.1f} us per step; "
        f"(a) = {ring_us:.1f} us.",
        "",
        "Expectation: (b - c) near (a) -- "
        + ("holds" if near else "DOES NOT HOLD") + " (within half of (a) or 5 us) -- "
        "and well under (d - c) -- " + ("holds" if under else "DOES NOT HOLD")
        + " (under half of it).  Reported, not gated.",
        "",
    ]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
