"""What the tests of the ray queries and profiles/tools/ray_query_time.py share
(no test in here)."""
import os
import re

import numpy as np

from madrona_amd.simlib import REPO_ROOT


def lidar_table():
    """kLidarCos / kLidarSin of sims/escape_room_phys/sim.cpp, float32 [30, 3]
    (cos, sin, 0): the literals, parsed as the compiler parses them."""
    text = open(os.path.join(REPO_ROOT, "sims", "escape_room_phys", "sim.cpp")).read()
    cols = []
    for name in ("kLidarCos", "kLidarSin"):
        body = re.search(name + r"\[consts::numLidarSamples\]\s*=\s*\{(.*?)\}", text, re.S).group(1)
        cols.append(np.array([np.float32(v.rstrip("f")) for v in re.findall(r"-?[\d.]+f", body)],
                             np.float32))
    assert len(cols[0]) == len(cols[1]) == 30
    return np.stack([cols[0], cols[1], np.zeros(30, np.float32)], -1)
