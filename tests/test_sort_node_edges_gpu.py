"""GPU: the sort node (SortArchetypeNode / CompactArchetypeNode,
madrona_amd/csrc/sort_archetype.hip) at shapes set on purpose, against numpy.

sims/sort_stress with flag 32 exports a per-world Plan that its LoadPlan task
graph applies: item count (0..40), how the keys are set (KEY_MODES), which
items are then destroyed without compaction (their rows stay, WorldID -1).
Flag 64 exports Item's Vec3 column, a pinned column the sort must keep in
place and copy the sorted rows back into.  Each case then

  * runs the key sort (KeySort: SortArchetypeNode<Item, Key> + a ResetTmpAlloc
    the batch may carry) once through mwhip_profile: every column dumped raw
    must equal the one before gathered with np.argsort(keys, kind="stable");
  * runs the world sort (WorldSort: CompactArchetypeNode<Item> + ResetTmpAlloc)
    the same way: a stable sort by WorldID with the destroyed rows dropped,
    per-world counts as np.bincount;
  * after each, Probe reads every held item's Key through its entity handle;
  * sorts an already sorted table again: every column bit-identical;
  * re-sizes every world without compaction (PlanResize: rows destroyed inside
    the world-sorted prefix, new rows appended behind it -- the input the
    compaction chain is built for) and checks the world sort of that table;
  * asserts from the profile's kernel roles and grids that the sort took the
    path the case names (single launch, radix chain with its pass count,
    compaction chain, grid rounds, gather variant, pinned copy-back, carried
    ResetTmpAlloc).

Every sort runs through mwhip_profile and never through a replay, so the
executor's between-replay heuristics (sortsOutgrown) cannot move a table to
another path in the middle of a case."""
from dataclasses import dataclass

import numpy as np
import pytest

from madrona_amd.simlib import Simulator, hip_lib_path

pytestmark = pytest.mark.gpu

LOAD_PLAN, KEY_SORT, WORLD_SORT, PROBE, PLAN_RESIZE = 4, 5, 6, 7, 8
FLAG_PLAN, FLAG_PINNED = 32, 64
MAX_ITEMS = 40
KEY_MODES = ["random", "equal", "two", "top_byte", "low_byte", "ascending",
             "descending", "all_ones", "zero_or_ones"]

# sort_archetype.hip
SORT_TILE = 2048
SMALL_BUILD_ROWS = 32768 // 4       # single launch while rows * 4 <= the limit


def world_passes(worlds: int) -> int:
    """sortNumPasses for a world sort: W ids and the all-ones key distinct."""
    return ((worlds + 1).bit_length() + 7) // 8


@dataclass
class Case:
    worlds: int
    rows: int                       # table rows LoadPlan leaves (destroyed included)
    dist: str = "even"              # even | first | last | alternate
    mode: str = "random"
    destroy: str = "none"           # none | some | all
    small: str = "1"                # MADRONA_MWHIP_SORT_SMALL
    compact: str = "1"              # MADRONA_MWHIP_SORT_COMPACT
    grid: str = ""                  # MADRONA_MWHIP_SORT_MAX_GRID (unset: "")
    carry: str = "1"                # MADRONA_MWHIP_SORT_CARRIES_MISC
    pinned: bool = False
    regrow: str = "churn"           # second phase: churn (+-6) | fill (40) | drain (0)
    param: int = 0x5A3C96E1

    @property
    def id(self) -> str:
        parts = [f"w{self.worlds}", f"n{self.rows}", self.dist, self.mode]
        if self.destroy != "none":
            parts.append(f"destroy-{self.destroy}")
        parts.append(f"small{self.small}")
        parts.append(f"compact{self.compact}")
        if self.grid:
            parts.append(f"grid{self.grid}")
        if self.carry != "1":
            parts.append("nocarry")
        if self.pinned:
            parts.append("pinned")
        if self.regrow != "churn":
            parts.append(self.regrow)
        return "-".join(parts)


def _cases():
    cs = []
    # table rows at the tile edges, the single-launch limit and beyond, both
    # through the single launch and through the chains
    for n, w in [(0, 1), (1, 1), (2047, 64), (2048, 64), (2049, 64), (4097, 128)]:
        cs.append(Case(w, n, destroy="some" if n > 1 else "none"))
        cs.append(Case(w, n, small="0", destroy="some" if n > 1 else "none"))
    cs.append(Case(300, 768, mode="two", compact="2"))
    cs.append(Case(300, 8192, small="1", compact="2"))
    cs.append(Case(300, 8193, small="1", compact="2"))
    cs.append(Case(1024, 16384, destroy="some", compact="2"))
    cs.append(Case(1024, 16385, destroy="some", compact="2"))
    for n in (32767, 32768, 32769):
        cs.append(Case(1024, n, destroy="some"))
    cs.append(Case(1024, 32769, destroy="some", compact="2"))
    cs.append(Case(2600, 100000, destroy="some"))
    cs.append(Case(2600, 100000, destroy="some", compact="2", pinned=True))
    # world counts around the pass-count steps, one item per world
    for w in (254, 255, 256):
        cs.append(Case(w, w, small="0", destroy="some"))
        cs.append(Case(w, w, small="0", compact="2"))
    cs.append(Case(65534, 65534, destroy="some"))
    cs.append(Case(65535, 65535, destroy="some"))
    cs.append(Case(65535, 65535, mode="equal", compact="2"))
    # distributions over the worlds
    cs.append(Case(300, 40, dist="first", small="0"))
    cs.append(Case(300, 40, dist="last", small="0", compact="2"))
    cs.append(Case(300, 40, dist="first"))
    cs.append(Case(1000, 15000, dist="alternate"))
    cs.append(Case(1000, 15000, dist="alternate", compact="2", mode="two"))
    cs.append(Case(1000, 20000, destroy="all"))
    cs.append(Case(1000, 20000, destroy="all", compact="2"))
    cs.append(Case(64, 2000, destroy="all"))
    # every key mode on the radix chain (key sort and the order the world sort
    # must keep) and through the single launch
    for m in KEY_MODES:
        cs.append(Case(1000, 25000, mode=m, destroy="some"))
        cs.append(Case(100, 3000, mode=m, destroy="some"))
    for m in ("equal", "top_byte", "ascending", "zero_or_ones"):
        cs.append(Case(1000, 25000, mode=m, destroy="some", compact="2"))
    # chain knobs on tables of many tiles
    for compact in ("0", "1", "2"):
        for grid in ("", "1", "3"):
            cs.append(Case(2000, 40000, destroy="some", compact=compact, grid=grid,
                           mode="two" if grid else "random"))
    for compact in ("0", "2"):
        cs.append(Case(1500, 30000, destroy="some", compact=compact, pinned=True))
    cs.append(Case(1500, 30000, destroy="some", grid="3", mode="low_byte"))
    cs.append(Case(80, 2500, destroy="some"))
    for carry in ("0", "1"):
        cs.append(Case(1000, 20000, destroy="some", carry=carry))
        cs.append(Case(1000, 20000, destroy="some", carry=carry, compact="2"))
        cs.append(Case(50, 1500, destroy="some", carry=carry))
    # second phase: long tails (more than sortCompactTailLimit rows behind the
    # prefix), whole prefixes destroyed
    cs.append(Case(1024, 16384, compact="2", regrow="fill"))
    cs.append(Case(1024, 16384, compact="2", grid="3", regrow="fill", pinned=True))
    cs.append(Case(1024, 16384, compact="0", regrow="fill"))
    cs.append(Case(1024, 30000, compact="2", regrow="drain"))
    cs.append(Case(1024, 30000, compact="1", regrow="drain"))
    cs.append(Case(200, 4000, compact="2", regrow="fill"))
    cs.append(Case(200, 4000, compact="2", small="0", regrow="fill"))
    # pinned column through the single launch and the radix chain
    cs.append(Case(50, 1500, destroy="some", pinned=True))
    cs.append(Case(1000, 20000, destroy="some", pinned=True, mode="equal"))
    cs.append(Case(1000, 20000, destroy="some", pinned=True, small="0", grid="3"))
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cs


CASES = _cases()


def _plan(case: Case):
    """Per-world plan rows (count, mode, param, destroyLo, destroyHi) and the
    per-world item counts."""
    w, n = case.worlds, case.rows
    counts = np.zeros(w, dtype=np.int64)
    if case.dist == "even":
        targets = np.arange(w)
    elif case.dist == "alternate":
        targets = np.arange(0, w, 2)
    elif case.dist == "first":
        targets = np.array([0])
    elif case.dist == "last":
        targets = np.array([w - 1])
    else:
        raise ValueError(case.dist)
    base, extra = divmod(n, len(targets))
    counts[targets] = base
    counts[targets[:extra]] += 1
    assert counts.sum() == n and counts.max(initial=0) <= MAX_ITEMS, case.id

    rng = np.random.default_rng(case.worlds * 7919 + n)
    masks = np.zeros(w, dtype=np.uint64)
    for i in range(MAX_ITEMS):
        if case.destroy == "all":
            hit = counts > i
        elif case.destroy == "some":
            hit = (counts > i) & (rng.random(w) < 0.3)
        else:
            break
        masks |= hit.astype(np.uint64) << np.uint64(i)
    plan = np.zeros((w, 5), dtype=np.uint32)
    plan[:, 0] = counts
    plan[:, 1] = KEY_MODES.index(case.mode)
    plan[:, 2] = case.param
    plan[:, 3] = (masks & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    plan[:, 4] = (masks >> np.uint64(32)).astype(np.uint32)
    destroyed = sum(bin(int(m)).count("1") for m in masks)
    return plan.view(np.int32), counts, destroyed


class Table:
    """Item's columns in table order (destroyed rows included)."""

    def __init__(self, s: Simulator, cols, rows: int):
        self.names = [s.columns[i][0] for i in cols]
        self.cols = {name: s.dump_column_raw(i, max(rows, 1))
                     for name, i in zip(self.names, cols)}
        self.n = len(self.cols["Item.Key"])
        for name, c in self.cols.items():
            assert len(c) == self.n, name

    @property
    def keys(self):
        return self.cols["Item.Key"].view(np.uint32).ravel()

    @property
    def worlds(self):
        return self.cols["Item.WorldID"].view(np.int32).ravel()

    @property
    def entities(self):
        return self.cols["Item.Entity"].view(np.uint32).reshape(-1, 2)  # gen, id

    def assert_equals(self, other: "Table", perm, what):
        assert self.n == len(perm), (what, self.n, len(perm))
        for name in self.names:
            assert np.array_equal(self.cols[name], other.cols[name][perm]), (what, name)


def _roles(stats):
    return [(k["name"].rsplit(":", 1)[-1], k["workgroups"]) for k in stats
            if ":sort." in k["name"] or k["name"].startswith("misc:")]


def _check_path(case: Case, stats, world_sort: bool, rows: int, build_rows=None):
    """rows: the table's rows now; build_rows: when its graph was built."""
    roles = _roles(stats)
    names = [r for r, _ in roles]
    misc = ["clear/reset"] if case.carry == "0" else []
    build_rows = rows if build_rows is None else build_rows
    if case.small != "0" and build_rows <= SMALL_BUILD_ROWS:
        assert names == ["sort.small"] + misc, (world_sort, roles)
        return "small"
    tail = ["sort.gather"] + (["sort.finalize"] if case.pinned else []) + misc
    tiles = -(-rows // SORT_TILE)
    if world_sort and case.compact == "2":
        assert names == ["sort.compact.prepare", "sort.compact.scatter"] + tail, roles
        grids = [g for r, g in roles if r == "sort.compact.scatter"]
        path = "compact"
    else:
        passes = world_passes(case.worlds) if world_sort else 4
        assert names == ["sort.histogram"] + ["sort.onesweep"] * passes + tail, roles
        grids = [g for r, g in roles if r == "sort.onesweep"]
        path = f"radix{passes}"
    if case.grid:
        # rounds: tile = workgroup + round * grid
        assert all(g == int(case.grid) for g in grids), roles
        assert int(case.grid) < tiles, (case.grid, tiles)
        path += f"-grid{case.grid}"
    else:
        assert all(g >= tiles for g in grids), (roles, tiles)
    return path


def _regrow(case: Case, live_per_world):
    rng = np.random.default_rng(case.worlds * 31 + case.rows)
    if case.regrow == "fill":
        target = np.full(case.worlds, MAX_ITEMS)
    elif case.regrow == "drain":
        target = np.zeros(case.worlds, dtype=np.int64)
    else:
        target = np.clip(live_per_world + rng.integers(-6, 7, case.worlds), 0, MAX_ITEMS)
    plan = np.zeros((case.worlds, 5), dtype=np.int32)
    plan[:, 0] = target
    created = int(np.maximum(target - live_per_world, 0).sum())
    destroyed = int(np.maximum(live_per_world - target, 0).sum())
    return plan, created, destroyed


def _check_probe(s: Simulator, case: Case, table: Table, what):
    probe = s.read_tensor("probe")
    live = table.worlds >= 0
    held = probe[:, 0]
    assert held.sum() == live.sum(), (what, held.sum(), live.sum())
    if held.sum() == 0:
        return
    ent = probe[:, 2:].reshape(case.worlds, MAX_ITEMS, 3).view(np.uint32)
    slot = np.arange(MAX_ITEMS)[None, :] < held[:, None]
    gen, eid, key = ent[..., 0][slot], ent[..., 1][slot], ent[..., 2][slot]
    world = np.repeat(np.arange(case.worlds), held)
    # row of every live entity id in the dump
    row_of = np.full(int(table.entities[live, 1].max()) + 1, -1, dtype=np.int32)
    live_rows = np.nonzero(live)[0]
    row_of[table.entities[live_rows, 1]] = live_rows
    assert (eid < len(row_of)).all(), what
    rows = row_of[eid]
    assert (rows >= 0).all(), (what, "entity handle reaches no live row")
    assert np.array_equal(table.entities[rows, 0], gen), (what, "generation")
    assert np.array_equal(table.worlds[rows], world), (what, "world")
    assert np.array_equal(table.keys[rows], key), (what, "Key through the handle")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_sort_node_edges(built, monkeypatch, case):
    monkeypatch.setenv("MADRONA_MWHIP_SORT_SMALL", case.small)
    monkeypatch.setenv("MADRONA_MWHIP_SORT_COMPACT", case.compact)
    monkeypatch.setenv("MADRONA_MWHIP_SORT_CARRIES_MISC", case.carry)
    if case.grid:
        monkeypatch.setenv("MADRONA_MWHIP_SORT_MAX_GRID", case.grid)
    else:
        monkeypatch.delenv("MADRONA_MWHIP_SORT_MAX_GRID", raising=False)

    plan, counts, destroyed = _plan(case)
    flags = FLAG_PLAN | (FLAG_PINNED if case.pinned else 0)
    with Simulator(hip_lib_path("sort_stress"), case.worlds, seed=3, flags=flags) as s:
        cols = [i for i, (name, _, _) in enumerate(s.columns) if name.startswith("Item.")]
        key_col = [i for i in cols if s.columns[i][0] == "Item.Key"][0]
        s.write_tensor("plan", plan)
        s.run_taskgraph(LOAD_PLAN)
        key_graph = s.taskgraph_graph(KEY_SORT)
        world_graph = s.taskgraph_graph(WORLD_SORT)
        probe_graph = s.taskgraph_graph(PROBE)
        pin_ptr = s.tensor_ptr("item_vec3") if case.pinned else None

        def check_pinned(table, what):
            if not case.pinned:
                return
            assert s.tensor_ptr("item_vec3") == pin_ptr, what
            exported = s.read_tensor("item_vec3")[: table.n]
            assert np.array_equal(exported.view(np.uint8).reshape(table.n, 12),
                                  table.cols["Item.Vec3"]), what

        # ---- the table as planned -----------------------------------------
        pre = Table(s, cols, case.rows)
        assert pre.n == case.rows
        assert (pre.worlds == -1).sum() == destroyed
        if case.mode == "ascending":
            assert (np.diff(pre.keys.astype(np.int64)) > 0).all()
        if case.mode == "descending":
            assert (np.diff(pre.keys.astype(np.int64)) < 0).all()

        # ---- key sort --------------------------------------------------------
        key_path = _check_path(case, s.profile(reps=1, graph=key_graph), False,
                               case.rows)
        post = Table(s, cols, case.rows)
        perm = np.argsort(pre.keys, kind="stable")
        post.assert_equals(pre, perm, "key sort")
        assert (post.keys[:-1] <= post.keys[1:]).all()
        check_pinned(post, "key sort")
        s.profile(reps=1, graph=probe_graph)
        _check_probe(s, case, post, "key sort")

        # ---- world sort (compaction) -------------------------------------------
        world_path = _check_path(case, s.profile(reps=1, graph=world_graph), True,
                                 case.rows)
        live = case.rows - destroyed
        comp = Table(s, cols, live)
        wkeys = post.worlds.view(np.uint32)
        wperm = np.argsort(wkeys, kind="stable")
        wperm = wperm[wkeys[wperm] != 0xFFFFFFFF]
        comp.assert_equals(post, wperm, "world sort")
        assert (comp.worlds >= 0).all()
        same = comp.worlds[:-1] == comp.worlds[1:]
        assert (comp.keys[:-1][same] <= comp.keys[1:][same]).all(), "key order in a world"
        _, per_world = s.dump_column(key_col, MAX_ITEMS)
        assert np.array_equal(per_world, np.bincount(comp.worlds, minlength=case.worlds))
        check_pinned(comp, "world sort")
        s.profile(reps=1, graph=probe_graph)
        _check_probe(s, case, comp, "world sort")

        # ---- sorting a sorted table changes nothing ----------------------------
        s.profile(reps=1, graph=key_graph)
        again = Table(s, cols, live)
        again.assert_equals(comp, np.argsort(comp.keys, kind="stable"), "key sort 2")
        s.profile(reps=1, graph=key_graph)
        twice = Table(s, cols, live)
        twice.assert_equals(again, np.arange(live), "key sort of a key-sorted table")
        s.profile(reps=1, graph=world_graph)
        s.profile(reps=1, graph=world_graph)
        rest = Table(s, cols, live)
        rest.assert_equals(comp, np.arange(live), "world sort of a world-sorted table")
        check_pinned(rest, "idempotence")
        s.profile(reps=1, graph=probe_graph)
        _check_probe(s, case, rest, "idempotence")

        # ---- new rows behind the world-sorted prefix, holes in it ---------------
        plan2, created, destroyed2 = _regrow(case, per_world)
        s.write_tensor("plan", plan2)
        s.run_taskgraph(PLAN_RESIZE)
        rows2 = live + created
        grown = Table(s, cols, rows2)
        assert grown.n == rows2 and (grown.worlds == -1).sum() == destroyed2
        stats = s.profile(reps=1, graph=world_graph)
        if world_path == "small" and _roles(stats)[0][0] != "sort.small":
            # (the replay may have sent a busy small table to the chain,
            # runtime_state.hip sortsOutgrown)
            regrow_path = _check_path(case, stats, True, rows2, SMALL_BUILD_ROWS + 1)
        else:
            regrow_path = _check_path(case, stats, True, rows2,
                                      0 if world_path == "small" else case.rows)
        live2 = rows2 - destroyed2
        final = Table(s, cols, live2)
        gkeys = grown.worlds.view(np.uint32)
        gperm = np.argsort(gkeys, kind="stable")
        final.assert_equals(grown, gperm[gkeys[gperm] != 0xFFFFFFFF], "regrow world sort")
        _, per_world2 = s.dump_column(key_col, MAX_ITEMS)
        assert np.array_equal(per_world2, plan2[:, 0])
        assert np.array_equal(per_world2, np.bincount(final.worlds, minlength=case.worlds))
        check_pinned(final, "regrow")
        s.profile(reps=1, graph=probe_graph)
        _check_probe(s, case, final, "regrow")

    print(f"{case.id}: key sort {key_path}, world sort {world_path}, "
          f"after {case.regrow} ({created} new rows, {destroyed2} destroyed) "
          f"{regrow_path}")
