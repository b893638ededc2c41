"""What makes test_bvh_edges_gpu.py trustworthy, without a GPU: the reference
backend on the plan-mode worlds of sims/broadphase_only (DESIGN.md "Broadphase
plan mode") against plain restatements (bvh_edges_utils.py).

* The reference's rays and box queries against a float64 brute force over the
  axis-aligned cubes of the still layouts: the reference pinned independently
  of either tree.
* Conditions on the inputs: the reference's build neither checks the node index
  it hands out against its node array nor the depth of its 64-entry stack, so
  every planned (layout, L, max_leaves) is run through a numpy restatement of
  the build and must stay inside both (and inside the 32 entries of the query
  stack).  The restatement is itself pinned to the reference: the leaf ids and
  the candidate order it predicts are the ones the reference produces.
* L = 0 and L = 1: the reference backend runs them cleanly (a tree of one empty
  node / one node with one leaf), so they stay in the lock step.
"""
import numpy as np
import pytest

import bvh_edges_utils as U
from madrona_amd.simlib import Simulator, ref_lib_path

SIM = "broadphase_only"
WORLDS = 56
STEPS = 12
SEED = 3

# every (layout, max_leaves mode, no-pillars) the plan can produce
ALL_CASES = [(layout, mode, False) for layout, mode in U.plan_cases()] + \
    [(layout, "64" if layout == "doubling" else "exact", True) for layout in U.LAYOUTS]
# the reference's answers do not depend on max_leaves: the brute force runs once
# per still layout, with and without pillars
BRUTE_CASES = [(layout, "64" if layout == "doubling" else "exact", nop)
               for layout in U.STILL_LAYOUTS for nop in (False, True)]

# Measured over BRUTE_CASES (steps 1, 6 and 12, about 128 000 rays): the reference's
# worst relative deviation of a hit distance from the float64 brute force.  It
# comes from the nested layout (cubes of up to 8.6 across entered a few
# millimetres from the sensor: an absolute float32 error of ~3e-7 on a distance
# of 3e-3); every other layout stays below 2.4e-7.  The bound is four times the
# measured value or 1e-6, whichever is larger.
MEASURED_T_DEVIATION = 9.441e-5
T_TOLERANCE = max(4.0 * MEASURED_T_DEVIATION, 1e-6)
GRAZING_CAP = 0.02


def _reference_dumps(layout, mode, no_pillars, steps=STEPS, worlds=WORLDS):
    if not U.plan_mode_built(ref_lib_path(SIM)):
        pytest.skip(f"reference backend of {SIM} absent from oracle/_ref, or built "
                    "from sources without the plan mode")
    flags = U.plan_flags(layout, mode, no_pillars)
    with Simulator(ref_lib_path(SIM), worlds, seed=SEED, num_workers=1,
                   flags=flags) as ref:
        for step in range(1, steps + 1):
            ref.step(1)
            yield step, U.dump_plan(ref)


def _case_id(case):
    return f"{case[0]}-{case[1]}" + ("-nopillars" if case[2] else "")


def _expected_leaf_ids(body, step):
    """Leaf ids by registration order: pillars then boxes at construction,
    boxes in reversed order then pillars from the first re-registration on."""
    n_box = int(body["dynamic"].sum())
    n_pil = len(body["dynamic"]) - n_box
    if step < U.PLAN_REBUILD_PERIOD:
        return np.concatenate([n_pil + np.arange(n_box), np.arange(n_pil)])
    return np.concatenate([n_box - 1 - np.arange(n_box), n_box + np.arange(n_pil)])


def _is_rebuild_step(step):
    return step == 1 or step % U.PLAN_REBUILD_PERIOD == 0


@pytest.mark.parametrize("case", ALL_CASES, ids=_case_id)
def test_planned_inputs_stay_inside_the_reference_build(case):
    """Node numbers <= numInternalNodes(max_leaves), build stack <= 64, query
    stack <= 32 for every world and every rebuild of the case, from a
    restatement that is pinned to the reference in the same pass: the predicted
    Box.LeafID / Pillar.LeafID equal the dumped ones, and for every body the
    candidates the reference emits are the leaves the restated tree's box query
    meets, in its order (pair order is traversal order, so this pins the tree
    shape and the permutation the swap partition leaves).

    Range records of the breadth-first device build (one per node, staged
    worlds: L <= 64 and node capacity <= 85): the largest count over all
    planned cases is 49 (drift, L = 63), against maxRebuildRanges = 96 --
    and no legal input can need more than 85, since a record is a node and the
    node bound above holds.  The -1 fallback of rebuildStagedSegmented is
    unreachable from legal inputs."""
    layout, mode, no_pillars = case
    seen_leaves = set()
    staged_peak_nodes = 0
    for step, dump in _reference_dumps(layout, mode, no_pillars):
        if not _is_rebuild_step(step):
            continue
        # still layouts: steps 8 and 12 rebuild the same leaves as step 4
        if layout != "drift" and step > U.PLAN_REBUILD_PERIOD:
            continue
        bodies = U.world_bodies(dump)
        cand = U.candidate_ids(dump, local_rows=True)
        cand_start = np.concatenate(
            [[0], np.cumsum(dump["Candidates.CandidateCollision"][1])])
        for w, body in enumerate(bodies):
            leaves, pillars, _, cap = U.plan_world(w, layout, mode, no_pillars)
            assert len(body["id"]) == leaves and (~body["dynamic"]).sum() == pillars
            seen_leaves.add(leaves)
            assert np.array_equal(body["leaf"], _expected_leaf_ids(body, step)), (step, w)

            by_leaf = np.argsort(body["leaf"])
            p_min, p_max = U.leaf_boxes(body["pos"][by_leaf], body["scale"][by_leaf],
                                        body["vel"][by_leaf])
            centres = ((p_min + p_max) / np.float32(2)).astype(np.float32)
            tree = U.restated_build(centres)

            where = (case, step, w, leaves, cap)
            assert len(tree["nodes"]) <= U.num_internal_nodes(cap), where
            assert tree["peak_stack"] <= 64, where
            assert tree["peak_traversal_stack"] <= 32, where
            if leaves <= 64 and U.num_internal_nodes(cap) <= 85:
                staged_peak_nodes = max(staged_peak_nodes, len(tree["nodes"]))

            # ---- the restatement pinned to the reference ----
            n_lo, n_hi = U.node_boxes(tree, p_min, p_max)
            boxes = (p_min.tolist(), p_max.tolist(), n_lo.tolist(), n_hi.tolist())
            ids_by_leaf = body["id"][by_leaf]
            dyn_by_leaf = body["dynamic"][by_leaf]
            predicted = {}
            for leaf in range(leaves):
                a = int(ids_by_leaf[leaf])
                met = U.query_leaves(tree, boxes, boxes[0][leaf], boxes[1][leaf])
                assert leaf in met
                predicted[a] = [int(ids_by_leaf[b]) for b in met
                                if a < ids_by_leaf[b] and
                                (dyn_by_leaf[leaf] or dyn_by_leaf[b])]
            rows = cand[cand_start[w]:cand_start[w + 1]]
            assert np.all(rows[:, 0] == w)
            got = {}
            order_of_a = []
            for _, a, b in rows.tolist():
                if a not in got:
                    # (a body's pairs are contiguous)
                    assert not order_of_a or order_of_a[-1] != a
                    got[a] = []
                    order_of_a.append(a)
                else:
                    assert order_of_a[-1] == a, where
                got[a].append(b)
            for a, want in predicted.items():
                assert got.get(a, []) == want, (where, a)
    assert seen_leaves == set(U.LEAF_TABLE)
    assert staged_peak_nodes <= 85 < 96


def test_doubling_at_exact_size_would_overrun_the_node_array():
    """Why the doubling layout is restricted: twelve leaves at 1, 2, 4, ... with
    max_leaves = 12 number 17 nodes where the reference allocates 16 (it never
    checks).  The plan gives those worlds max_leaves = 64."""
    centres = np.zeros((12, 3), np.float32)
    centres[:, 0] = [2.0 ** i / 64 for i in range(12)]
    tree = U.restated_build(centres)
    assert U.num_internal_nodes(12) == 16
    assert len(tree["nodes"]) > 16
    assert len(tree["nodes"]) <= U.num_internal_nodes(64)


def test_restated_split_rules():
    """The tie rules by hand: equal x and y extents fall through to z; a pivot
    that leaves one side empty cuts at n // 2; one leaf is cut into none and
    one; an empty range is a node of its own."""
    # 5 coincident leaves: halves 2 + 3, quarters 1 1 1 2, input order kept
    tree = U.restated_build(np.zeros((5, 3), np.float32))
    assert [len(n["children"]) for n in tree["nodes"]] == [4, 1, 1, 1, 2]
    # (the query pushes the root's four children and pops the last one first)
    assert tree["traversal"] == [3, 4, 2, 1, 0]
    # 5 leaves, one far along x: the half split leaves 4 + 1, the single leaf
    # is cut into an empty range (a node without children) and a range of one
    c = np.zeros((5, 3), np.float32)
    c[2, 0] = 8
    tree = U.restated_build(c)
    sizes = [len(n["children"]) for n in tree["nodes"]]
    assert sizes == [4, 2, 2, 0, 1] and tree["order"][-1] == 2
    # equal x and y extents, z all equal: the pivot is the common z, nothing is
    # below it, the cut falls back to n // 2 and the order stays
    c = np.array([[0, 0, 1], [1, 1, 1], [0, 1, 1], [1, 0, 1], [0, 0, 1], [1, 1, 1]],
                 np.float32)
    assert U.restated_build(c)["order"] == [0, 1, 2, 3, 4, 5]
    # a strictly larger x extent does split along x (swap partition)
    c[1, 0] = 2
    assert U.restated_build(c)["order"] != [0, 1, 2, 3, 4, 5]
    assert U.restated_build(np.zeros((0, 3), np.float32))["nodes"] == \
        [{"parent": -1, "children": []}]


def _brute_force_case(layout, mode, no_pillars, steps):
    """Worst relative t deviation, rays checked, rays left out as grazing."""
    dirs = U.fan_directions()
    worst, checked, grazing = 0.0, 0, 0
    for step, dump in _reference_dumps(layout, mode, no_pillars, max(steps)):
        if step not in steps:
            continue
        bodies = U.world_bodies(dump)
        sensors = U.world_sensors(dump)
        for w, (body, (s_pos, fan, plain)) in enumerate(zip(bodies, sensors)):
            centre = body["pos"].astype(np.float64)
            half = body["scale"].astype(np.float64) * 0.5
            for s in range(len(s_pos)):
                t_ref = fan[s, :32].view(np.float32)
                e_ref = fan[s, 32:64]
                # the plain rays are the same rays through the same function
                for k, i in enumerate(U.PLAIN_RAYS):
                    assert plain[s, k] == fan[s, i] and plain[s, 8 + k] == fan[s, 32 + i]
                for i in range(32):
                    where = (layout, no_pillars, step, w, s, i)
                    if len(centre) == 0:
                        assert e_ref[i] == -1, where
                        checked += 1
                        continue
                    if U.ray_is_grazing(s_pos[s], dirs[i], centre, half):
                        grazing += 1
                        continue
                    checked += 1
                    t = U.brute_force_ray(s_pos[s], dirs[i], centre, half)
                    if not np.isfinite(t).any():
                        assert e_ref[i] == -1, where
                        continue
                    t_min = t.min()
                    assert e_ref[i] >= 0, (where, t_min)
                    dev = abs(float(t_ref[i]) - t_min) / t_min
                    worst = max(worst, dev)
                    assert dev <= T_TOLERANCE, (where, float(t_ref[i]), t_min)
                    hit = np.nonzero(body["id"] == e_ref[i])[0]
                    assert len(hit) == 1, where
                    # (coincident boxes tie: any box at the closest distance)
                    assert t[hit[0]] <= t_min * (1 + T_TOLERANCE), (where, t[hit[0]], t_min)
    return worst, checked, grazing


@pytest.mark.parametrize("case", BRUTE_CASES, ids=_case_id)
def test_reference_rays_against_float64_brute_force(case):
    """Every ray of the fan at steps 1, 6 and 12: the closest entry into any
    cube by the slab test in float64 against the reference's RayFan -- the same
    entity (any of the tied ones where boxes coincide), t within T_TOLERANCE,
    "nothing" exactly where nothing is entered within reach.  A ray that starts
    inside a cube does not meet that cube (the reference reports entries only).
    Grazing rays (bvh_edges_utils.ray_is_grazing) are left out and stay under
    2 % of all rays (measured: 8 of 10 656 at most, 0.08 %).

    Measured worst relative deviation of the reference's t from float64:
    9.441e-5 (nested; below 2.4e-7 on every other layout), so T_TOLERANCE is
    3.78e-4."""
    worst, checked, grazing = _brute_force_case(*case, steps=(1, 6, 12))
    print(f"{_case_id(case)}: worst relative t deviation {worst:.3e}, "
          f"{checked} rays checked, {grazing} grazing")
    assert checked > 0
    assert grazing < GRAZING_CAP * (checked + grazing)


@pytest.mark.parametrize("case", BRUTE_CASES, ids=_case_id)
def test_reference_box_queries_against_brute_force(case):
    """Probe32 / Probe64 of the reference (both from findEntitiesWithinAABB):
    the reported entity is a dynamic body whose extents overlap the query box;
    "none" exactly when no dynamic body does.  The all-containing box finds a
    body in every world that has a box."""
    layout, mode, no_pillars = case
    f = np.float32
    for step, dump in _reference_dumps(layout, mode, no_pillars):
        bodies = U.world_bodies(dump)
        sensors = U.world_sensors(dump)
        p32 = dump["Prober.Probe32"][0].view(np.int32).reshape(-1, 4)
        p64 = dump["Prober.Probe64"][0].view(np.int32).reshape(-1, 4)
        assert np.array_equal(p32, p64)
        assert len(p32) == WORLDS
        for w, (body, (s_pos, _, _)) in enumerate(zip(bodies, sensors)):
            dyn = body["dynamic"]
            first_box = body["pos"][0] if dyn.any() else np.zeros(3, f)
            centres = [first_box, s_pos[0], s_pos[-1], s_pos[0]]
            half_body = body["scale"] * f(0.5)
            lo, hi = body["pos"] - half_body, body["pos"] + half_body
            for k in range(4):
                q_lo = centres[k] - f(U.PROBE_HALF[k])
                q_hi = centres[k] + f(U.PROBE_HALF[k])
                inside = dyn & np.all(hi > q_lo, axis=1) & np.all(q_hi > lo, axis=1)
                where = (case, step, w, k)
                if not inside.any():
                    assert p32[w, k] == -1, where
                else:
                    assert p32[w, k] in body["id"][inside], where
            if dyn.any():
                assert p32[w, 3] >= 0, (case, step, w)


@pytest.mark.parametrize("layout", ["drift", "line", "lattice", "doubling"])
def test_box_query_answers_lie_beyond_the_first_window(layout):
    """The 32-lane wave query takes the leaves in traversal order, 32 per
    window.  On these layouts the lock step really needs its later windows:
    some worlds' answers are leaves at rank >= 32 of the restated traversal
    order (the query boxes sit at the first box, which the traversal -- last
    pushed node first -- reaches late).  The coincident, outlier and nested
    layouts are answered from the first window."""
    mode = "64" if layout == "doubling" else "exact"
    late = 0
    for step, dump in _reference_dumps(layout, mode, False, steps=1):
        p32 = dump["Prober.Probe32"][0].view(np.int32).reshape(-1, 4)
        for w, body in enumerate(U.world_bodies(dump)):
            if len(body["id"]) <= 32:
                continue
            by_leaf = np.argsort(body["leaf"])
            p_min, p_max = U.leaf_boxes(body["pos"][by_leaf], body["scale"][by_leaf],
                                        body["vel"][by_leaf])
            tree = U.restated_build(((p_min + p_max) / np.float32(2)).astype(np.float32))
            rank = {int(body["id"][by_leaf][leaf]): r
                    for r, leaf in enumerate(tree["traversal"])}
            late += sum(1 for k in range(4)
                        if p32[w, k] >= 0 and rank[int(p32[w, k])] >= 32)
    assert late >= 10, (layout, late)


def test_reference_runs_empty_and_single_leaf_worlds():
    """L = 0 and L = 1 on the reference backend: it builds a root without
    children / with one leaf and every query walks it: no hit, no pair, no
    probe result for L = 0; the one box is seen from above and found by the
    queries for L = 1.  They stay in the lock step of test_bvh_edges_gpu.py."""
    for layout in ("coincident", "drift"):
        hits_one = 0
        for step, dump in _reference_dumps(layout, "exact", False):
            bodies = U.world_bodies(dump)
            sensors = U.world_sensors(dump)
            counts = dump["Candidates.CandidateCollision"][1]
            p32 = dump["Prober.Probe32"][0].view(np.int32).reshape(-1, 4)
            for w in range(WORLDS):
                leaves = U.LEAF_TABLE[w % len(U.LEAF_TABLE)]
                if leaves > 1:
                    continue
                assert len(bodies[w]["id"]) == leaves and counts[w] == 0
                _, fan, plain = sensors[w]
                if leaves == 0:
                    assert np.all(fan[:, 32:64] == -1) and np.all(plain[:, 8:16] == -1)
                    assert np.all(fan[:, :32] == 0)
                    assert np.all(p32[w] == -1)
                else:
                    hits_one += int((fan[:, 32:64] == bodies[w]["id"][0]).sum())
                    assert p32[w, 3] == bodies[w]["id"][0]
        assert hits_one > 0
