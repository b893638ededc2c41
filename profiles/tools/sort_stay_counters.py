#!/usr/bin/env python3
"""Stay-mode counters of the sort node (Simulator.sort_stats()) over steady-state
steps of a bench workload: per sorted table, the share of compaction runs that
stayed in place and the rows the gather copied per run.

    python profiles/tools/sort_stay_counters.py [sim worlds [steps]] > stay_counters.json

Default: escape_room_phys at 8192 worlds (the headline), 300 steps after 700."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import bench  # noqa: E402
from madrona_amd.simlib import Simulator, hip_lib_path  # noqa: E402


def main():
    sim_name = sys.argv[1] if len(sys.argv) > 1 else "escape_room_phys"
    worlds = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    with Simulator(hip_lib_path(sim_name), worlds, seed=5, gpu_id=0, flags=200) as sim:
        bench.fill_actions(sim_name, sim, worlds, 0, 99)
        sim.step_async(700)
        torch.cuda.synchronize()
        before = sim.sort_stats()
        sim.step_async(steps)
        torch.cuda.synchronize()
        sim.sync()
        after = sim.sort_stats()
    tables = {}
    for arch, st in after.items():
        d = {k: v - before.get(arch, {}).get(k, 0) for k, v in st.items()}
        runs = max(d["runs"], 1)
        d["stay_share"] = round(d["stay_runs"] / runs, 4)
        d["rows_copied_per_run"] = round(d["rows_copied"] / runs, 1)
        d["rows_out_per_run"] = round(d["rows_out"] / runs, 1)
        tables[str(arch)] = d
    json.dump({"sim": sim_name, "worlds": worlds, "steps": steps,
               "auto_reset": "p = 1/200 per world per step", "tables": tables},
              sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
