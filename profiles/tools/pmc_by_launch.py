#!/usr/bin/env python3
"""rocprofv3 --pmc counters per LAUNCH SITE of the kernels matching PATTERN, from
a rocpd database (rocprofv3 --kernel-trace --pmc ... -d DIR -o NAME).

A kernel that a step launches more than once (bvhRefreshKernel<true, ..>: behind
the movement system and behind the reset) is split by the matching kernel that
was dispatched before it, which tells its launch sites apart.

    python profiles/tools/pmc_by_launch.py out.db 'bvhRefresh|grabQuery'"""
import re
import sqlite3
import sys
from collections import defaultdict

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from summarize_pmc import short_name  # noqa: E402


def main():
    db = sqlite3.connect(sys.argv[1])
    pattern = sys.argv[2]
    rows = db.execute(
        "select dispatch_id, kernel_name, counter_name, value, grid_size_x, "
        "workgroup_size_x, vgpr_count, lds_block_size "
        "from counters_collection order by dispatch_id").fetchall()
    per_dispatch = {}
    for did, kname, cname, value, grid, wg, vgpr, lds in rows:
        if not re.search(pattern, kname):
            continue
        d = per_dispatch.setdefault(did, {"kernel": short_name(kname),
                                          "shape": (grid, wg, vgpr, lds), "c": {}})
        d["c"][cname] = d["c"].get(cname, 0.0) + value
    acc = defaultdict(lambda: {"n": 0, "c": defaultdict(float), "shape": None})
    prev = "-"
    for did in sorted(per_dispatch):
        d = per_dispatch[did]
        a = acc[(d["kernel"], prev)]
        a["n"] += 1
        a["shape"] = d["shape"]
        for cname, value in d["c"].items():
            a["c"][cname] += value
        prev = d["kernel"]
    for (kernel, after), a in sorted(acc.items()):
        if a["n"] < 5:
            continue        # (the seams between the bench's phases)
        grid, wg, vgpr, lds = a["shape"]
        print(f"{kernel}\n    dispatched after {after}: n={a['n']} grid={grid} "
              f"workgroup={wg} arch_vgpr={vgpr} lds={lds}")
        for cname, total in sorted(a["c"].items()):
            print(f"    {cname:24s} avg/launch {total / a['n']:16.1f}")


if __name__ == "__main__":
    main()
