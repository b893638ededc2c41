"""Step time of the mesh_cast simulator (sims/mesh_cast) at N worlds, per
kernel (Simulator.profile), next to the steps/s of the reference CPU backend's
speed build of the same simulator on this box's cores -- the stated baseline,
a measurement and not a target.  Writes profiles/mesh_cast_w<N>.json:
    python profiles/tools/mesh_cast_time.py [worlds] [out.json]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from madrona_amd.simlib import Simulator, hip_lib_path, ref_lib_path

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
    REPO, "profiles", f"mesh_cast_w{W}.json")
AGENTS = 4

result = {"sim": "mesh_cast", "worlds": W, "agents_per_world": AGENTS,
          "queries_per_agent_step": {"traceRay": 16, "sphereCast": 1, "findOverlaps": 1}}

with Simulator(hip_lib_path("mesh_cast"), W, seed=5) as hip:
    hip.step(50)
    t0 = time.perf_counter()
    hip.step(200)
    wall = (time.perf_counter() - t0) / 200
    kernels = {}
    for k in hip.profile(20):
        kernels[k["name"]] = kernels.get(k["name"], 0.0) + k["avg_us"]
    result["hip"] = {
        "step_us_kernels": round(sum(kernels.values()), 2),
        "step_us_wall": round(wall * 1e6, 2),
        "world_steps_per_s_wall": round(W / wall),
        "kernels_us": {n: round(v, 2) for n, v in sorted(kernels.items(),
                                                         key=lambda x: -x[1])},
    }

path = ref_lib_path("mesh_cast", speed=True)
if os.path.exists(path):
    cores = len(os.sched_getaffinity(0))
    with Simulator(path, W, seed=5, num_workers=0) as ref:
        ref.step(5)
        t0 = time.perf_counter()
        ref.step(5)
        per_step = (time.perf_counter() - t0) / 5
        n = int(max(10, min(2000, 6.0 / max(per_step, 1e-6))))
        t0 = time.perf_counter()
        ref.step(n)
        per_step = (time.perf_counter() - t0) / n
    result["cpu_baseline"] = {
        "what": "reference CPU backend, speed build, all cores of this box",
        "cores": cores, "steps_timed": n,
        "step_us_wall": round(per_step * 1e6, 2),
        "world_steps_per_s_wall": round(W / per_step),
    }
else:
    result["cpu_baseline"] = None

with open(OUT, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result))
