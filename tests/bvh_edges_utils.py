"""Helpers of the broadphase edge tests (test_bvh_edges_cpu.py,
test_bvh_edges_gpu.py, test_parity_gpu.py): the plan mode of
sims/broadphase_only (flag encoding and leaf table, as in its sim.hpp), the
candidate pairs of a dump, and three plain restatements used as references:

* the leaf boxes the BVH keeps for a body (float32, the reference's operations
  in the reference's order: broadphase.cpp:440-485),
* the reference's top-down build over leaf centres (broadphase.cpp:47-240) with
  the traversal order of its box query (include/madrona/broadphase.inl:22-59),
* a float64 brute force of the closest ray hit and of the box queries over
  axis-aligned cubes.
"""
from __future__ import annotations

import functools
import os

import numpy as np

# ---- plan mode (sims/broadphase_only/sim.hpp) -------------------------------

LEAF_TABLE = [0, 130, 1, 97, 2, 66, 3, 65, 4, 64, 5, 63, 6, 62, 8, 61, 9, 60, 16, 33,
              17, 32, 20, 31, 21, 129, 96, 128]
LAYOUTS = {"drift": 0, "coincident": 1, "line": 2, "lattice": 3, "outlier": 4,
           "nested": 5, "doubling": 6}
STILL_LAYOUTS = [name for name in LAYOUTS if name != "drift"]
MAX_LEAVES_MODES = {"exact": 0, "64": 1, "65": 2}
DOUBLING_MAX_LEAVES = 12
PLAN_REBUILD_PERIOD = 4
PLAIN_RAYS = [0, 1, 2, 3, 4, 9, 18, 27]
PROBE_HALF = [0.4, 1.0, 3.0, 50.0]
RAY_T_MAX = 40.0
MAX_PAIRS = 16384         # 130 coincident boxes make 8385 pairs
MAX_ROWS = 256            # every other table: at most 130 rows per world


def dump_plan(sim):
    """Simulator.dump_all with a row bound per table: only the candidate table
    needs room for thousands of rows per world (a common bound would ask for
    600 MB for the 640-byte ray fans)."""
    return {name: sim.dump_column(i, MAX_PAIRS if name.startswith("Candidates.")
                                  else MAX_ROWS)
            for i, (name, _, _) in enumerate(sim.columns)}


@functools.lru_cache(maxsize=None)
def plan_mode_built(lib_path: str) -> bool:
    """True if the reference-backend simulator library at lib_path exists and
    was built from sources that have the plan mode (it exports the plan mode's
    columns): oracle/_ref is built apart from the tree and may be older."""
    from madrona_amd.simlib import Simulator
    if not os.path.exists(lib_path):
        return False
    with Simulator(lib_path, 1, seed=1, num_workers=1) as sim:
        return "Prober.Probe32" in [name for name, _, _ in sim.columns]


def plan_flags(layout: str, max_leaves: str = "exact", no_pillars: bool = False) -> int:
    return 2 | (4 if no_pillars else 0) | (MAX_LEAVES_MODES[max_leaves] << 4) | \
        (LAYOUTS[layout] << 8)


def plan_cases():
    """(layout, max_leaves mode) the tests run: doubling is defined for
    max_leaves = 64 alone (the simulator forces it for its doubling worlds)."""
    cases = [(layout, mode) for layout in LAYOUTS if layout != "doubling"
             for mode in MAX_LEAVES_MODES]
    return cases + [("doubling", "64")]


def plan_world(global_world: int, layout: str, max_leaves: str, no_pillars=False):
    """(leaves, pillars, effective layout, max_leaves handed to the BVH)."""
    leaves = LEAF_TABLE[global_world % len(LEAF_TABLE)]
    pillars = 4 if leaves >= 8 and not no_pillars else 0
    if layout == "doubling":
        if leaves <= DOUBLING_MAX_LEAVES:
            max_leaves = "64"
        else:
            layout = "line"
    cap = max(leaves, 1)
    if leaves <= 64 and max_leaves in ("64", "65"):
        cap = int(max_leaves)
    return leaves, pillars, layout, cap


def num_internal_nodes(num_leaves: int) -> int:
    """BVH::numInternalNodes: the size of the node array for max_leaves."""
    return max((num_leaves - 1 + 2) // 3, 1) + num_leaves


def fan_directions() -> np.ndarray:
    """The 32 directions of plan mode's ray fan, float64, unit length."""
    out = np.zeros((32, 3))
    axis = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1)]
    for i in range(32):
        if i < 5:
            out[i] = axis[i]
        else:
            d = np.array([(i * 7) % 11 - 5 + 0.5, (i * 3) % 13 - 6 + 0.25,
                          0.75 * (i % 5 - 2)])
            out[i] = d / np.linalg.norm(d)
    return out


# ---- dumps ------------------------------------------------------------------

def candidate_pairs(dump, arch_names):
    """CandidateCollision rows -> (world, entity id a, entity id b, aPrim, bPrim).
    A Loc's row is world-local on the CPU backend and global on the GPU; both are
    resolved through the dumped Entity columns (grouped by world, world order)."""
    cand, cand_counts = dump["Candidates.CandidateCollision"]
    cand = cand.view(np.int32).reshape(-1, 6)      # a.arch a.row b.arch b.row aPrim bPrim
    tables = {}
    for arch_id, name in arch_names.items():
        ents, counts = dump[f"{name}.Entity"]
        ids = ents.view(np.int32).reshape(-1, 2)[:, 1]
        tables[arch_id] = (ids, np.concatenate([[0], np.cumsum(counts)]))
    out = []
    world_of_row = np.repeat(np.arange(len(cand_counts)), cand_counts)
    for row, w in zip(cand, world_of_row):
        pair = []
        for arch, r in ((row[0], row[1]), (row[2], row[3])):
            ids, starts = tables[int(arch)]
            local_guess = starts[w] + r           # CPU: world-local row
            global_guess = r                      # GPU: global row
            pair.append((int(ids[local_guess]) if local_guess < len(ids) else -1,
                         int(ids[global_guess]) if global_guess < len(ids) else -1))
        out.append((int(w), pair, int(row[4]), int(row[5])))
    return out, cand_counts


def candidate_ids(dump, local_rows: bool):
    """Candidate pairs as an int array [rows, 3]: world, entity id a, entity id b
    (vectorised candidate_pairs for the big plan worlds).  Archetype ids: Box is
    the smaller one (registered first)."""
    cand, counts = dump["Candidates.CandidateCollision"]
    cand = cand.view(np.int32).reshape(-1, 6)
    world = np.repeat(np.arange(len(counts)), counts)
    if len(cand) == 0:
        return np.zeros((0, 3), np.int64)
    box_arch = min(cand[:, 0].min(), cand[:, 2].min())
    ids = {}
    for name in ("Box", "Pillar"):
        ents, n = dump[f"{name}.Entity"]
        ids[name] = (ents.view(np.int32).reshape(-1, 2)[:, 1],
                     np.concatenate([[0], np.cumsum(n)]))
    # (a world with pillars always has boxes too, so box_arch is Box's id
    # whenever two archetype ids occur)
    assert len(set(cand[:, 0]) | set(cand[:, 2])) <= 2
    out = np.empty((len(cand), 3), np.int64)
    out[:, 0] = world
    for k, (arch_col, row_col) in enumerate(((0, 1), (2, 3))):
        is_box = cand[:, arch_col] == box_arch
        res = np.empty(len(cand), np.int64)
        for name, sel in (("Box", is_box), ("Pillar", ~is_box)):
            table, starts = ids[name]
            rows = cand[sel, row_col].astype(np.int64)
            if local_rows:
                rows = rows + starts[world[sel]]
            res[sel] = table[rows]
        out[:, 1 + k] = res
    return out


PILLAR_POS = np.array([[-2.5, -2.5, 1.0], [2.5, -2.5, 1.0], [-2.5, 2.5, 1.0],
                       [2.5, 2.5, 1.0]], np.float32)
PILLAR_SCALE = np.array([1.0, 1.0, 2.0], np.float32)


def world_bodies(dump):
    """Per world: dict of entity ids, positions, scales, velocities (float32),
    leaf ids and the dynamic flag of its bodies, boxes first (table order), then
    pillars."""
    def rows(col, dtype, width):
        data, counts = dump[col]
        return data.view(dtype).reshape(-1, width), np.concatenate([[0], np.cumsum(counts)])

    b_ent, b_start = rows("Box.Entity", np.int32, 2)
    b_pos, _ = rows("Box.Position", np.float32, 3)
    b_scale, _ = rows("Box.Scale", np.float32, 3)
    b_vel, _ = rows("Box.Velocity", np.float32, 6)
    b_leaf, _ = rows("Box.LeafID", np.int32, 1)
    p_ent, p_start = rows("Pillar.Entity", np.int32, 2)
    p_leaf, _ = rows("Pillar.LeafID", np.int32, 1)
    worlds = []
    for w in range(len(b_start) - 1):
        b = slice(b_start[w], b_start[w + 1])
        p = slice(p_start[w], p_start[w + 1])
        n_p = p.stop - p.start
        worlds.append({
            "id": np.concatenate([b_ent[b, 1], p_ent[p, 1]]),
            "pos": np.concatenate([b_pos[b], PILLAR_POS[:n_p]]),
            "scale": np.concatenate([b_scale[b], np.tile(PILLAR_SCALE, (n_p, 1))]),
            "vel": np.concatenate([b_vel[b, :3], np.zeros((n_p, 3), np.float32)]),
            "leaf": np.concatenate([b_leaf[b, 0], p_leaf[p, 0]]),
            "dynamic": np.concatenate([np.ones(b.stop - b.start, bool),
                                       np.zeros(n_p, bool)]),
        })
    return worlds


def world_sensors(dump):
    """Per world: sensor positions float32 [n, 3], RayFan int32 view [n, 160]
    (32 t, 32 entity, 96 normal) and RayFanPlain int32 view [n, 40]."""
    pos, counts = dump["Sensor.Position"]
    pos = pos.view(np.float32).reshape(-1, 3)
    fan = dump["Sensor.RayFan"][0].view(np.int32).reshape(-1, 160)
    plain = dump["Sensor.RayFanPlain"][0].view(np.int32).reshape(-1, 40)
    start = np.concatenate([[0], np.cumsum(counts)])
    return [(pos[start[w]:start[w + 1]], fan[start[w]:start[w + 1]],
             plain[start[w]:start[w + 1]]) for w in range(len(counts))]


# ---- the leaf boxes (float32) -----------------------------------------------

def leaf_boxes(pos, scale, vel):
    """The boxes BVH::updateLeafPosition stores for unit cubes with identity
    rotation: pos -/+ scale / 2, grown along the velocity by 2 dt v and on both
    sides by 100 dt^2 (expandAABBWithMotion), float32 throughout."""
    f = np.float32
    dt = f(0.05)
    vel_factor = f(2.0) * dt
    accel = f(100.0) * dt * dt
    half = scale.astype(f) * f(0.5)
    p_min = pos.astype(f) - half
    p_max = pos.astype(f) + half
    delta = vel_factor * vel.astype(f)
    min_delta = delta - accel
    max_delta = delta + accel
    p_min = np.where(min_delta < 0, p_min + min_delta, p_min).astype(f)
    p_max = np.where(max_delta > 0, p_max + max_delta, p_max).astype(f)
    return p_min, p_max


# ---- the reference's build, restated ----------------------------------------
#
# Restated from the reference's src/physics/broadphase.cpp:47-240 (BVH::rebuild)
# in this project's own words:
#
# The build works on a list of leaf ids (initially 0 .. n-1) and a stack of
# pending ranges (at most 64 entries; the reference never checks).  A range of at
# most four leaves -- an EMPTY range too -- becomes a node holding those leaves.
# A longer range gets its node number first, is cut in two by split(), each
# half is cut again by split(), and the four quarters are pushed so that they
# are built left to right; the range's entry stays on the stack below them and
# is popped once they are done.  Every node but the root is appended, when it
# is finished, to the first free child slot of its parent with the union of its
# children's boxes.  Nodes are numbered in the order they are first met; the
# reference never compares that number with the size of its node array.
#
# split(range): the bounds of the leaf centres of the range; the axis is x if
# the x extent is STRICTLY greater than both others, else y if the y extent is
# strictly greater than both others, else z.  The pivot is the midpoint of the
# centre bounds on that axis.  Partition by swapping: walk from the left past
# centres below the pivot, from the right past centres at or above it, swap
# the two leaves the walks stop at, continue until the walks meet.  The cut is
# where they met, unless that is either end of the range: then it is n // 2.
# A range of one leaf is therefore cut into an empty part and a part of one.

def restated_build(centres):
    """centres: float32 [n, 3] by leaf id.  Returns a dict: nodes (list of
    {parent, children: [('leaf', id) | ('node', id)]}), order (leaf ids after
    the partitions), peak_stack, traversal (leaf ids in the order an unpruned
    box query meets them), peak_traversal_stack."""
    centres = np.asarray(centres, np.float32).reshape(-1, 3)
    n = len(centres)
    order = list(range(n))
    f = np.float32

    def split(base, count):
        if count == 0:
            return 0
        c = centres[order[base:base + count]]
        lo, hi = c.min(axis=0), c.max(axis=0)
        ext = (hi - lo).astype(f)
        if ext[0] > ext[1] and ext[0] > ext[2]:
            axis = 0
        elif ext[1] > ext[0] and ext[1] > ext[2]:
            axis = 1
        else:
            axis = 2
        pivot = f(0.5) * f(lo[axis] + hi[axis])
        left, right = 0, count
        while left < right:
            while left < right and centres[order[base + left]][axis] < pivot:
                left += 1
            while left < right and centres[order[base + right - 1]][axis] >= pivot:
                right -= 1
            if left < right:
                i, j = base + left, base + right - 1
                order[i], order[j] = order[j], order[i]
                left += 1
                right -= 1
        return left if 0 < left < count else count // 2

    nodes = []
    stack = [{"node": -1, "parent": -1, "lo": 0, "n": n}]
    peak = 1
    while stack:
        top = stack[-1]
        if top["n"] <= 4:
            node = len(nodes)
            nodes.append({"parent": top["parent"], "children":
                          [("leaf", order[top["lo"] + i]) for i in range(top["n"])]})
        elif top["node"] < 0:
            node = len(nodes)
            top["node"] = node
            nodes.append({"parent": top["parent"], "children": []})
            lo, cnt = top["lo"], top["n"]
            half = split(lo, cnt)
            q1 = split(lo, half)
            q3 = split(lo + half, cnt - half)
            for c_lo, c_n in ((lo + half + q3, cnt - half - q3), (lo + half, q3),
                              (lo + q1, half - q1), (lo, q1)):
                stack.append({"node": -1, "parent": node, "lo": c_lo, "n": c_n})
            peak = max(peak, len(stack))
            continue
        else:
            node = top["node"]
        stack.pop()
        parent = nodes[node]["parent"]
        if parent >= 0:
            nodes[parent]["children"].append(("node", node))

    # the box query: a stack of node ids (32 entries in the reference), the
    # children of a node in slot order, leaves reported at once, nodes pushed
    traversal, visit, peak_visit = [], [0], 1
    while visit:
        node = nodes[visit.pop()]
        for kind, idx in node["children"]:
            if kind == "leaf":
                traversal.append(idx)
            else:
                visit.append(idx)
        peak_visit = max(peak_visit, len(visit))
    return {"nodes": nodes, "order": order, "peak_stack": peak,
            "traversal": traversal, "peak_traversal_stack": peak_visit}


def node_boxes(tree, p_min, p_max):
    """Union boxes of every node of a restated tree (float32 min / max are
    exact); a node without leaves below it gets the reference's invalid box."""
    big = np.finfo(np.float32).max
    lo = np.full((len(tree["nodes"]), 3), big, np.float32)
    hi = np.full((len(tree["nodes"]), 3), -big, np.float32)
    for idx in range(len(tree["nodes"]) - 1, -1, -1):      # children have larger ids
        for kind, c in tree["nodes"][idx]["children"]:
            c_lo, c_hi = (p_min[c], p_max[c]) if kind == "leaf" else (lo[c], hi[c])
            lo[idx] = np.minimum(lo[idx], c_lo)
            hi[idx] = np.maximum(hi[idx], c_hi)
    return lo, hi


def overlaps(a_lo, a_hi, b_lo, b_hi):
    """AABB::overlaps of the reference: strict, boxes that only touch do not
    overlap (the line layout has such pairs)."""
    return (a_lo[0] < b_hi[0] and a_lo[1] < b_hi[1] and a_lo[2] < b_hi[2] and
            b_lo[0] < a_hi[0] and b_lo[1] < a_hi[1] and b_lo[2] < a_hi[2])


def query_leaves(tree, boxes, q_lo, q_hi):
    """Leaf ids a box query reports, in its order, right after a rebuild (slot
    boxes are the leaf boxes / the union boxes).  boxes: leaf min, leaf max,
    node min, node max as lists of float triples (float32 values are exact in
    Python floats)."""
    p_min, p_max, n_lo, n_hi = boxes
    out, visit = [], [0]
    while visit:
        for kind, c in tree["nodes"][visit.pop()]["children"]:
            if kind == "leaf":
                if overlaps(q_lo, q_hi, p_min[c], p_max[c]):
                    out.append(c)
            elif overlaps(q_lo, q_hi, n_lo[c], n_hi[c]):
                visit.append(c)
    return out


# ---- float64 brute force ------------------------------------------------------

def brute_force_ray(origin, direction, centre, half):
    """Entry distance of a ray into each axis-aligned box (float64 slab test);
    inf where it misses, starts inside, or enters beyond RAY_T_MAX."""
    o = np.asarray(origin, np.float64)
    d = np.asarray(direction, np.float64)
    c = np.asarray(centre, np.float64).reshape(-1, 3)
    h = np.asarray(half, np.float64).reshape(-1, 3)
    t_in = np.full(len(c), -np.inf)
    t_out = np.full(len(c), np.inf)
    miss = np.zeros(len(c), bool)
    for a in range(3):
        if d[a] == 0.0:
            miss |= np.abs(o[a] - c[:, a]) >= h[:, a]
            continue
        t1 = (c[:, a] - h[:, a] - o[a]) / d[a]
        t2 = (c[:, a] + h[:, a] - o[a]) / d[a]
        t_in = np.maximum(t_in, np.minimum(t1, t2))
        t_out = np.minimum(t_out, np.maximum(t1, t2))
    hit = ~miss & (t_in <= t_out) & (t_in >= 0.0) & (t_in <= RAY_T_MAX)
    return np.where(hit, t_in, np.inf)


GRAZE = 1e-4


def ray_is_grazing(origin, direction, centre, half):
    """True if growing or shrinking some box by GRAZE changes whether the ray
    meets it (it passes within GRAZE of an edge or face plane, or starts that
    close to a face), or if its closest hit lies that close to RAY_T_MAX."""
    half = np.asarray(half, np.float64).reshape(-1, 3)
    big = brute_force_ray(origin, direction, centre, half + GRAZE)
    small = brute_force_ray(origin, direction, centre, half - GRAZE)
    if np.any(np.isfinite(big) != np.isfinite(small)):
        return True
    t = brute_force_ray(origin, direction, centre, half)
    return bool(np.isfinite(t).any() and abs(t.min() - RAY_T_MAX) < 1e-3)
