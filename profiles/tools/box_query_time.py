"""Time of a box query compute (mwhip_boxes_compute_async) on escape_room_phys,
8192 worlds, after 50 steps: 2 bundles per world (the agents, their centres fed
from a world view of Agent.Position with the view's counts) of 1 box and of 8
boxes per bundle (half extents 0.5 .. 8, doubling every other box), 16 hits per
box, in both mappings (cooperative, the default, and packed).  The two mappings'
words are compared before anything is timed.  Next to them the simulator's own
grabQuerySystem node from mwhip_profile (the average of 20 profiled steps of
the same simulator): a related but not identical job -- one box per agent, the
first accepted entity, no list -- so it is context, not a bar.
Each figure is the median of REPS repetitions, each timed with a pair of HIP
events on the executor's own stream around one compute_async, after WARM untimed
repetitions, with the stream idle in between.  No threshold.  Writes
profiles/box_query_times.md:
    python profiles/tools/box_query_time.py [worlds] [out.md]"""
import ctypes as C
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "box_query_times.md")
SIM, STEPS, DENOM, SEED = "escape_room_phys", 50, 200, 5
A, HITS = 2, 16
REPS, WARM = 20, 3


def hip_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> hipError {rc}")


def main():
    import torch    # (its HIP runtime is the one every library of the process binds to)
    if not torch.cuda.is_available():
        raise SystemExit("box_query_time.py measures on the GPU; none is visible")
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
    with Simulator(hip_lib_path(SIM), W, seed=SEED, flags=DENOM) as sim, \
            sim.world_view("Agent", ["Agent.Position"], max_rows=A) as view:
        sim.step(STEPS)
        view.compute()
        stream = C.c_void_p(sim.stream())
        source = dict(centre=(view.buffer_ptr("Agent.Position"), 12, 0), bundles_per_world=A,
                      count=(view.counts_ptr, 4, 0))
        for per_bundle in (1, 8):
            half = np.float32([0.5 * 2 ** (g // 2) for g in range(per_bundle)])
            half = np.tile(np.repeat(half[:, None], 3, axis=1), (W * A, 1))
            outs = {}
            for packed in (False, True):
                with sim.box_query(W * A, per_bundle, HITS, packed=packed, **source) as query:
                    device = query.lo().device
                    query.lo().copy_(torch.from_numpy(-half).to(device))
                    query.hi().copy_(torch.from_numpy(half).to(device))
                    torch.cuda.synchronize()
                    query.compute()
                    outs[packed] = (query.status().cpu().numpy(), query.counts().cpu().numpy(),
                                    query.hits().cpu().numpy())
                    rows.append((per_bundle, "packed" if packed else "cooperative",
                                 int(outs[packed][1].sum()), timed(stream, query.compute_async)))
                    sim.sync()
            for a, b in zip(outs[False], outs[True]):
                assert np.array_equal(a, b), "the two mappings disagree"
        stats = sim.profile(20)
        node = [k for k in stats if "grabQuerySystem" in k["name"]]
        assert len(node) == 1, [k["name"] for k in stats]

    device_name = (f"{torch.cuda.get_device_name(0)} "
                   f"({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})")
    lines = [
        "# Box queries: compute time",
        "",
        f"Written by `profiles/tools/box_query_time.py` on: {device_name}.",
        "",
        f"Shape: `{SIM}`, {W} worlds, seed {SEED}, auto-reset 1/{DENOM}, after {STEPS} steps; "
        f"{W * A} bundles (the agents, centres from a world view of Agent.Position) of 1 and "
        f"of 8 boxes, half extents 0.5 .. 8, {HITS} hits per box.  The two mappings' status, "
        "count and hits are equal word for word.",
        "",
        f"Each query: median of {REPS} (min - max), after {WARM} untimed repetitions, each timed "
        "with two HIP events on the executor's stream around one compute_async, the stream "
        "idle before it.  The node: its avg_us in mwhip_profile over 20 profiled steps of the "
        "same simulator (it is the parent commit's: this change does not touch it).",
        "",
        "| boxes per bundle | mapping | entities listed | us | min - max us |",
        "|---:|---|---:|---:|---:|"]
    for per_bundle, mapping, listed, (med, lo, hi) in rows:
        lines.append(f"| {per_bundle} | {mapping} | {listed} | {med:.1f} | {lo:.1f} - {hi:.1f} |")
    lines += [
        f"| | `{node[0]['name']}` in the step (mwhip_profile) | | {node[0]['avg_us']:.1f} | |",
        "",
        "Reported, not gated.  grabQuerySystem asks one box per agent for the first entity "
        "it accepts and lists nothing: context, not a bar.", ""]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
