"""Time of a contact query compute (mwhip_contacts_compute_async) on
escape_room_phys, 8192 worlds, after 50 steps, 32 contacts per world: both
mappings (cooperative, the default, and plain -- every pair through the generic
single-lane routine, one at a time) x both pose modes (solver, current).  The two
mappings' words are compared before anything is timed.  Next to them the
physics step kernels of the same simulator from mwhip_profile (the average of
20 profiled steps): a step runs the narrowphase four times (once per substep)
besides the solver, so it is context, not a bar.
Each figure is the median of REPS repetitions, each timed with a pair of HIP
events on the executor's own stream around one compute_async, after WARM untimed
repetitions, with the stream idle in between.  No threshold.  Writes
profiles/contact_query_times.md:
    python profiles/tools/contact_query_time.py [worlds] [out.md]"""
import ctypes as C
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles",
                                                         "contact_query_times.md")
SIM, STEPS, DENOM, SEED = "escape_room_phys", 50, 200, 5
K = 32
REPS, WARM = 20, 3


def hip_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> hipError {rc}")


def main():
    import torch    # (its HIP runtime is the one every library of the process binds to)
    if not torch.cuda.is_available():
        raise SystemExit("contact_query_time.py measures on the GPU; none is visible")
    runtime_lib()
    hip = C.CDLL("libamdhip64.so")
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

    rows = []
    with Simulator(hip_lib_path(SIM), W, seed=SEED, flags=DENOM) as sim:
        sim.step(STEPS)
        stream = C.c_void_p(sim.stream())
        for poses in ("solver", "current"):
            outs = {}
            for plain in (False, True):
                with sim.contact_query(K, poses=poses, plain=plain) as query:
                    query.compute()
                    torch.cuda.synchronize()
                    outs[plain] = [t.cpu().numpy() for t in (
                        query.status(), query.counts(), query.pairs(), query.num_points(),
                        query.normals(), query.points())]
                    assert (outs[plain][0] == 0).all()
                    rows.append((poses, "plain" if plain else "cooperative",
                                 int(outs[plain][1].sum()), int(outs[plain][1].max()),
                                 timed(stream, query.compute_async)))
                    sim.sync()
            for a, b in zip(outs[False], outs[True]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
                    "the two mappings disagree"
        stats = sim.profile(20)
        step = [k for k in stats if "physics:worldStep" in k["name"]]
        assert step, [k["name"] for k in stats]

    device_name = (f"{torch.cuda.get_device_name(0)} "
                   f"({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})")
    lines = [
        "# Contact queries: compute time",
        "",
        f"Written by `profiles/tools/contact_query_time.py` on: {device_name}.",
        "",
        f"Shape: `{SIM}`, {W} worlds, seed {SEED}, auto-reset 1/{DENOM}, after {STEPS} steps; "
        f"{K} contact slots per world.  The two mappings' status, count, pairs, num_points, "
        "normal and points are equal word for word in both pose modes.",
        "",
        f"Each query: median of {REPS} (min - max), after {WARM} untimed repetitions, each timed "
        "with two HIP events on the executor's stream around one compute_async, the stream "
        "idle before it.  The step kernels: their avg_us in mwhip_profile over 20 profiled "
        "steps of the same simulator (the parent commit's: this change does not touch them).",
        "",
        "| poses | mapping | contacts | most in a world | us | min - max us |",
        "|---|---|---:|---:|---:|---:|"]
    for poses, mapping, total, most, (med, lo, hi) in rows:
        lines.append(f"| {poses} | {mapping} | {total} | {most} | {med:.1f} | "
                     f"{lo:.1f} - {hi:.1f} |")
    for k in step:
        lines.append(f"| | `{k['name']}` in the step (mwhip_profile) | | | {k['avg_us']:.1f} | |")
    lines += [
        "",
        "Reported, not gated.  A step runs the narrowphase once per substep (four times) on the "
        "broadphase's candidates and solves; a query tests all pairs of a world once: context, "
        "not a bar.  The plain mapping sends the pairs through the generic routine one lane at "
        "a time, through one hull scratch per world: it is the yardstick, not a fast path.", ""]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
