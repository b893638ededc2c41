"""Time of a ray query compute (mwhip_rays_compute_async) at the BASELINE
configs[2] shape -- escape_room_phys, 8192 worlds, after 50 steps: 2 fans per
world (the agents) of 30 rays, origins and directions built from the agents'
Position and Rotation exactly as lidarSystem builds them, t_max 200 -- next to
the simulator's own lidarSystem node, which does the same casts inside the step
(its entry in mwhip_profile, the average of 20 profiled steps of the same
simulator; that node also looks up the EntityType of what it hit and stores
the samples).  The query's depths are checked against the exported lidar tensor
before anything is timed.
The query's figure is the median of REPS repetitions, each timed with a pair of
HIP events on the executor's own stream around one compute_async, after WARM
untimed repetitions, with the stream idle in between.  No threshold: both
figures and their ratio are reported.  Writes profiles/ray_query_times.md:
    python profiles/tools/ray_query_time.py [worlds] [out.md]"""
import ctypes as C
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from madrona_amd import ray_ref
from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "ray_query_times.md")
SIM, STEPS, DENOM, SEED = "escape_room_phys", 50, 200, 5
A, S, T_MAX = 2, 30, 200.0
REPS, WARM = 20, 3


def hip_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> hipError {rc}")


def main():
    import torch    # (its HIP runtime is the one every library of the process binds to)
    if not torch.cuda.is_available():
        raise SystemExit("ray_query_time.py measures on the GPU; none is visible")
    from ray_utils import lidar_table
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

    table = lidar_table()
    with Simulator(hip_lib_path(SIM), W, seed=SEED, flags=DENOM) as sim:
        sim.step(STEPS)
        stream = C.c_void_p(sim.stream())
        names = [c[0] for c in sim.columns]
        pos, counts = sim.dump_column(names.index("Agent.Position"), A)
        assert (counts == A).all()
        pos = pos.view(np.float32).reshape(W * A, 3)
        rot = sim.dump_column(names.index("Agent.Rotation"), A)[0].view(np.float32)
        rot = rot.reshape(W * A, 4)
        with sim.ray_query(W * A, S) as query:
            device = query.worlds().device
            query.worlds().copy_(torch.arange(W, dtype=torch.int32).repeat_interleave(A))
            query.origins().copy_(torch.from_numpy(pos + np.float32([0, 0, 0.5])).to(device))
            directions = ray_ref.normalize_f32(
                ray_ref.rotate_vec_f32(rot[:, None, :], table[None, :, :])).reshape(-1, 3)
            query.directions().copy_(torch.from_numpy(directions).to(device))
            query.t_max().fill_(T_MAX)
            torch.cuda.synchronize()
            query.compute()
            depth = query.hit_t().cpu().numpy() / np.float32(T_MAX)
            lidar = sim.read_tensor("lidar").reshape(-1, 2)
            assert np.array_equal(depth.view(np.int32), lidar[:, 0].copy().view(np.int32)), \
                "the query and the lidar node disagree"
            hits = int((query.status().cpu().numpy() == 1).sum())
            result = timed(stream, query.compute_async)
            sim.sync()
        stats = sim.profile(20)
        lidar_node = [k for k in stats if "lidarSystem" in k["name"]]
        assert len(lidar_node) == 1, [k["name"] for k in stats]
        node_us = lidar_node[0]["avg_us"]

    device_name = (f"{torch.cuda.get_device_name(0)} "
                   f"({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})")
    med, lo, hi = result
    lines = [
        "# Ray queries: compute time",
        "",
        f"Written by `profiles/tools/ray_query_time.py` on: {device_name}.",
        "",
        f"Shape: `{SIM}`, {W} worlds, seed {SEED}, auto-reset 1/{DENOM}, after {STEPS} steps "
        f"(BASELINE configs[2]); one query of {W * A} fans (the agents) of {S} rays = "
        f"{W * A * S} rays, origins and directions as lidarSystem builds them, t_max {T_MAX:g}; "
        f"{hits} rays hit.  The query's depths equal the exported lidar tensor bit for bit.",
        "",
        f"The query: median of {REPS} (min - max), after {WARM} untimed repetitions, each timed "
        "with two HIP events on the executor's stream around one compute_async, the stream "
        "idle before it.  The node: its avg_us in mwhip_profile over 20 profiled steps of the "
        "same simulator (the node is the parent commit's: this change does not touch it).",
        "",
        "| what | us | min - max us |",
        "|---|---:|---:|",
        f"| one compute of the ray query | {med:.1f} | {lo:.1f} - {hi:.1f} |",
        f"| `{lidar_node[0]['name']}` in the step (mwhip_profile) | {node_us:.1f} | |",
        f"| ratio (query / node) | {med / node_us:.2f} | |",
        "",
        "Reported, not gated.  The node does the same casts through the same "
        "BVH::traceRayShared, then reads the EntityType of each hit entity and stores the "
        "samples; the query stores hit_t, the Entity, the normal and a status per ray and "
        "reads its directions from memory instead of computing them.", ""]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
