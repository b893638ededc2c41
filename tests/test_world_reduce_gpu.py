"""-m gpu: world reduces (mwhip_reduce_*, Simulator.world_reduce()).

The yardstick is madrona_amd/reduce_ref.py, the definition in numpy, evaluated
over the table-order dump (dump_column_raw) and compared BIT FOR BIT: every
result of every term, every count and every alarm word; where the expected
float is a NaN both sides must be one.  Shapes are those at which the view
tests established their preconditions (sort_stress, 33 worlds, seed 7, the
Item table): every team size (1 .. 64 lanes per world) and plans of more
elements than lanes, a world whose rows straddle a 256-row block, several
worlds in one wavefront, empty worlds and tables, holes in the sorted prefix,
rows behind it and a table with no prefix at all.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from madrona_amd import reduce_ref
from madrona_amd.simlib import (RING_ON_STEP, ReduceTerm, Simulator, hip_lib_path, ref_lib_path,
                                runtime_lib)

pytestmark = pytest.mark.gpu

CHURN_ONLY = 1      # sort_stress: churn without the compaction behind it
SORT_BY_KEY = 2     # sort_stress: a sort of Item by Key (no world-sorted prefix is left)
RAW_CAP = 1 << 16   # rows a table-order dump has room for
SIX = ("sum", "min", "max", "absmax", "count_nonzero", "count_nonfinite")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_ref(sim):
    if not os.path.exists(ref_lib_path(sim)):
        pytest.skip("oracle/_ref missing on this box")


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _sort_stress(worlds=33, seed=7, flags=0):
    return Simulator(hip_lib_path("sort_stress"), worlds, seed=seed, flags=flags)


def _index(sim, name):
    return [c[0] for c in sim.columns].index(name)


def _raw_world_ids(sim, table="Item"):
    return sim.dump_column_raw(_index(sim, table + ".WorldID"), RAW_CAP).view(np.int32).ravel()


def _all_six(column, **options):
    return [(column, op, dict(options)) for op in SIX]


def _expected(sim, reduce, world_ids=None):
    """reduce_ref over the table-order dump: ([result per term], counts, alarm)"""
    if world_ids is None:
        world_ids = _raw_world_ids(sim, reduce.table)
    raws, results, counts = {}, [], None
    for column, term in reduce.terms:
        if column not in raws:
            raws[column] = sim.dump_column_raw(_index(sim, column), RAW_CAP)
            assert len(raws[column]) == len(world_ids), (column, len(raws[column]))
        result, counts = reduce_ref.reduce_of_raw(world_ids, raws[column], sim.num_worlds, term)
        results.append(result)
    return results, counts, reduce_ref.alarm_of(results, [t for _, t in reduce.terms])


def _got(reduce):
    reduce._sim.sync()
    return ([reduce.tensor(i).cpu().numpy() for i in range(len(reduce.terms))],
            reduce.counts.cpu().numpy(), reduce.alarm.cpu().numpy())


def _same(got, want, what, terms=None):
    got_results, got_counts, got_alarm = got
    want_results, want_counts, want_alarm = want
    assert got_counts.dtype == np.int32 and got_counts.shape == want_counts.shape
    bad = np.flatnonzero(got_counts != want_counts)
    assert len(bad) == 0, (what, "counts differ at worlds", bad[:4].tolist(),
                           got_counts[bad[:4]].tolist(), want_counts[bad[:4]].tolist())
    assert len(got_results) == len(want_results)
    for i, (g, w) in enumerate(zip(got_results, want_results)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, w.dtype, g.shape,
                                                           w.shape)
        g_bits, w_bits = g.view(np.uint32), w.view(np.uint32)
        differ = g_bits != w_bits
        if w.dtype == np.float32:
            # an expected NaN: both sides must be one (its payload is the adder's)
            differ &= ~(np.isnan(w) & np.isnan(g))
        bad = np.argwhere(differ)
        assert len(bad) == 0, (what, "term", i, terms[i] if terms else "", len(bad),
                               "results differ, first (world, elem):", bad[:4].tolist(),
                               [hex(int(g_bits[tuple(b)])) for b in bad[:4]],
                               [hex(int(w_bits[tuple(b)])) for b in bad[:4]])
    assert got_alarm.dtype == np.int32 and np.array_equal(got_alarm, want_alarm), \
        (what, "alarm", got_alarm.tolist(), want_alarm.tolist())


def _check(sim, reduce, what, world_ids=None):
    reduce.compute()
    want = _expected(sim, reduce, world_ids)
    _same(_got(reduce), want, what, reduce.terms)
    return want


def _fill_ff(reduce):
    torch = _torch()
    for i in range(len(reduce.terms)):
        reduce.tensor(i).view(torch.uint8).fill_(0xFF)
    reduce.counts.fill_(-1)
    reduce.alarm.fill_(-1)
    torch.cuda.synchronize()


# ---- 1. ops and dtypes ----------------------------------------------------------------
OPS_AND_DTYPES = (
    [("Item.Tag8", "sum"), ("Item.Tag8", "max"), ("Item.Tag8", "count_nonzero"),
     ("Item.Key", "sum"), ("Item.Key", "min"), ("Item.Key", "max")] +
    [("Item.Blob20", op, dict(dtype="i32", offset=8, elems=2)) for op in ("sum", "min", "max")] +
    _all_six("Item.Vec3") + _all_six("Item.Quad") +
    # (256 elements at most in a plan: Wide's 60 floats whole for two of the
    # ops, twenty of them, from three different offsets, for the other four)
    [("Item.Wide", "sum"), ("Item.Wide", "absmax"),
     ("Item.Wide", "min", dict(offset=0, elems=20)),
     ("Item.Wide", "max", dict(offset=80, elems=20)),
     ("Item.Wide", "count_nonzero", dict(offset=160, elems=20)),
     ("Item.Wide", "count_nonfinite", dict(offset=160, elems=20))])


def test_every_op_and_dtype_and_wave_shape(built):
    with _sort_stress() as s, s.world_reduce("Item", OPS_AND_DTYPES) as reduce:
        terms = [t for _, t in reduce.terms]
        assert [t.dtype for t in terms[:9]] == ["u8"] * 3 + ["u32"] * 3 + ["i32"] * 3
        assert [t.elems for t in terms[:9]] == [1] * 6 + [2] * 3
        assert all(t.dtype == "f32" for t in terms[9:])
        assert [t.elems for t in terms[9:]] == [3] * 6 + [4] * 6 + [60, 60, 20, 20, 20, 20]
        assert sum(t.elems for t in terms) == 254 and len(terms) == 27
        # result types; everything is zero at creation
        kinds = [reduce.tensor(i).cpu().numpy().dtype for i in range(27)]
        assert kinds[:9] == [np.uint32, np.uint32, np.int32] + [np.uint32] * 3 + [np.int32] * 3
        assert kinds[9:15] == [np.float32] * 4 + [np.int32] * 2
        assert not any(reduce.tensor(i).cpu().numpy().view(np.uint32).any() for i in range(27))
        assert not reduce.counts.cpu().numpy().any() and not reduce.alarm.cpu().numpy().any()

        straddles = three_in_a_wave = empty_world = False
        steps = 0
        for until in (0, 1, 7):
            s.step(until - steps)
            steps = until
            world = _raw_world_ids(s)
            # (after a full step the table is grouped by world, without holes)
            assert (np.diff(world) >= 0).all() and (world >= 0).all()
            results, counts, alarm = _check(s, reduce, ("step", until), world)
            assert counts.sum() == len(world) and counts.max() <= 40 and not alarm.any()
            ends = np.cumsum(counts.astype(np.int64))
            starts = ends - counts
            straddles |= bool(((counts > 0) & (starts // 256 != (ends - 1) // 256)).any())
            three_in_a_wave |= any(len(np.unique(world[at:at + 64])) >= 3
                                   for at in range(0, len(world), 64))
            empty_world |= bool((counts == 0).any())
            # (not vacuous: sums of Vec3 are neither zero nor all alike)
            assert len(np.unique(results[9][:, 0])) > 8
        assert straddles, "no world's Item rows straddle a 256-row block boundary"
        assert three_in_a_wave, "no 64-row stretch of Item holds rows of 3 worlds"
        assert empty_world, "no world without Item rows"


# ---- 2. team shapes -------------------------------------------------------------------
TEAM_SHAPES = {
    1: [("Item.Vec3", "sum", dict(offset=4, elems=1))],
    2: [("Item.Vec3", "sum", dict(elems=2))],
    3: [("Item.Vec3", "sum")],
    5: [("Item.Key", "max"), ("Item.Quad", "sum")],
    16: [("Item.Quad", op) for op in ("sum", "min", "max", "absmax")],
    60: [("Item.Wide", "sum")],
    64: [("Item.Wide", "sum"), ("Item.Quad", "absmax")],
    65: [("Item.Wide", "sum"), ("Item.Quad", "min"), ("Item.Tag8", "sum")],
    200: [("Item.Wide", "sum"), ("Item.Wide", "absmax"), ("Item.Wide", "count_nonzero"),
          ("Item.Blob20", "sum"), ("Item.Quad", "sum"), ("Item.Quad", "min"),
          ("Item.Quad", "max"), ("Item.Vec3", "sum")],
}


@pytest.mark.parametrize("elems", sorted(TEAM_SHAPES))
def test_team_shapes(built, elems):
    """1 .. 64 lanes per world (64 .. 1 worlds per wavefront), and plans whose
    elements a lane loops over."""
    with _sort_stress() as s, s.world_reduce("Item", TEAM_SHAPES[elems]) as reduce:
        assert sum(t.elems for _, t in reduce.terms) == elems
        s.step(2)
        world = _raw_world_ids(s)
        results, counts, _ = _check(s, reduce, ("elements", elems), world)
        assert counts.sum() == len(world) and (counts > 0).sum() > 16
        assert tuple(reduce.tensor(0).shape) == (33, reduce.terms[0][1].elems)
        assert results[0].any()


# ---- 3. special floats ----------------------------------------------------------------
def test_vec3_of_sort_stress_is_payload():
    """The column the next test poisons never reaches an index or a loop bound:
    the simulator only does arithmetic on it."""
    src = open(os.path.join(REPO, "sims", "sort_stress", "sim.cpp")).read()
    # every Vec3 of the source is bound to a variable called v3 or v
    bound = re.findall(r"Vec3 &(\w+)", src)
    assert bound and set(bound) <= {"v3", "v"}, bound
    element = r"\b(v3|v)\.v\["
    uses = [line.strip() for line in src.splitlines() if re.search(element, line)]
    assert len(uses) >= 7, uses
    for line in uses:
        # never inside the [...] of another access, a condition or a loop bound
        assert not re.search(r"\[[^\]]*" + element, line), line
        assert not re.search(r"\b(if|while|switch)\s*\(", line), line
        assert not re.search(r"\bfor\s*\([^)]*" + element, line), line
        assert not re.search(r"\?", line), line


def test_special_floats(built):
    torch = _torch()
    denormal = np.float32(1e-45)
    terms = [("Item.Vec3", op, dict(alarm=True, limit=1e7) if op in ("absmax", "count_nonfinite")
              else {}) for op in SIX]
    with _sort_stress() as s, s.world_reduce("Item", terms) as reduce, \
            s.world_view("Item", ["Item.Vec3"], max_rows=40) as view, \
            s.world_write("Item", ["Item.Vec3"], max_rows=40) as write:
        s.step(3)
        view.compute()
        counts = view.counts.cpu().numpy()
        a, b, c, d = [int(w) for w in np.flatnonzero(counts >= 4)[:4]]
        vec3 = view.tensor("Item.Vec3", np.float32).cpu().numpy().copy()
        # a: the order-sensitive rows and nothing else
        vec3[a] = 0.0
        vec3[a, :4, 0] = [1e8, 1.0, -1e8, 0.0]      # in row order 0; 1e8 - 1e8 first: 1
        vec3[a, :4, 1] = [1.0, 1e8, -1e8, 1.0]      # in row order 1; pairwise: 0
        vec3[a, :4, 2] = [1e8, -1e8, 1.0, 0.0]      # in row order 1; (1e8 + 1) first: 0
        # b: NaN, both infinities, a denormal and -0 among ordinary values
        vec3[b, 0] = [np.nan, np.inf, -0.0]
        vec3[b, 1] = [2.0, -np.inf, 0.0]
        vec3[b, 2] = [denormal, 1.0, -0.0]
        # c: only denormals, -0 and +0
        vec3[c] = [denormal, -0.0, 0.0]
        # d: zeros of both signs in both orders, and a column of NaNs
        vec3[d] = [0.0, 0.0, np.nan]
        vec3[d, 0] = [-0.0, 0.0, np.nan]
        vec3[d, 1] = [0.0, -0.0, np.nan]
        write.tensor("Item.Vec3", np.float32).copy_(torch.from_numpy(vec3).cuda())
        write.take.fill_(40)
        torch.cuda.synchronize()
        write.apply()

        results, _, alarm = _check(s, reduce, "special floats")
        by_op = dict(zip(SIX, results))
        bits = lambda x: x.view(np.uint32)      # noqa: E731
        # the values worked out by hand, so that the yardstick is not vacuous
        assert by_op["sum"][a].tolist() == [0.0, 1.0, 1.0]
        assert by_op["absmax"][a].tolist() == [1e8, 1e8, 1e8]
        assert np.isnan(by_op["sum"][b, 0]) and np.isnan(by_op["sum"][b, 1])
        assert by_op["absmax"][b, 1] == np.inf and by_op["min"][b, 1] == -np.inf
        assert by_op["max"][b, 1] == np.inf
        assert by_op["count_nonfinite"][b].tolist() == [1, 2, 0]
        assert by_op["min"][b, 0] <= float(denormal) and by_op["max"][b, 0] == 2.0
        assert bits(by_op["sum"][c])[0] == counts[c] and counts[c] >= 4
        assert bits(by_op["min"][c]).tolist() == [1, 0x80000000, 0]
        assert bits(by_op["max"][c]).tolist() == [1, 0x80000000, 0]
        assert by_op["count_nonzero"][c].tolist() == [counts[c], 0, 0]
        assert bits(by_op["min"][d]).tolist()[:2] == [0x80000000, 0]
        assert bits(by_op["max"][d]).tolist()[:2] == [0x80000000, 0]
        assert bits(by_op["min"][d])[2] == 0x7F800000 and bits(by_op["absmax"][d])[2] == 0
        assert by_op["count_nonfinite"][d].tolist() == [0, 0, counts[d]]
        assert by_op["count_nonzero"][d].tolist() == [0, 0, counts[d]]
        want_alarm = np.zeros(33, np.int32)
        want_alarm[[a, b, d]] = 1       # 1e8 > 1e7; NaN and Inf; NaN
        assert np.array_equal(alarm, want_alarm)


# ---- 4. holes, a tail, no prefix --------------------------------------------------------
HOLES_PLAN = (_all_six("Item.Vec3") + [("Item.Key", "sum"), ("Item.Key", "min"),
                                       ("Item.Tag8", "max"), ("Item.Wide", "sum"),
                                       ("Item.WorldID", "max", dict(dtype="i32")),
                                       ("Item.Entity", "min", dict(dtype="u32", elems=1))])


def test_holes_a_tail_and_no_prefix(built):
    with _sort_stress() as s, s.world_reduce("Item", HOLES_PLAN) as reduce:
        s.step(4)
        saw_hole = saw_descending = False
        for rnd in range(3):
            s.run_taskgraph(CHURN_ONLY)
            world = _raw_world_ids(s)
            saw_hole |= bool((world == -1).any())
            saw_descending |= bool((np.diff(world) < 0).any())
            results, counts, _ = _check(s, reduce, ("churn", rnd), world)
            # WorldID may be listed: its maximum over a world's rows is the world
            assert all(results[10][w, 0] == w for w in np.flatnonzero(counts))
        assert saw_hole, "no destroyed row (WorldID -1) in the raw table"
        assert saw_descending, "the raw world ids are non-decreasing"
        # no sorted prefix at all: rows of a world are scattered over the table
        s.run_taskgraph(SORT_BY_KEY)
        world = _raw_world_ids(s)
        live = world[world >= 0]
        assert (np.diff(live) < 0).sum() > len(live) // 4, "the key sort left the worlds grouped"
        _check(s, reduce, "sorted by key", world)
        # (this is the state dump_column refuses); after a full step both dumps agree
        s.step(1)
        results, counts, _ = _check(s, reduce, "after the next full step")
        for i, (column, term) in enumerate(reduce.terms):
            rows, per_world = s.dump_column(_index(s, column), 512)
            dumped, dumped_counts = reduce_ref.reduce_of_dump(rows, per_world, 33, term)
            assert np.array_equal(dumped_counts, counts), column
            assert np.array_equal(dumped.view(np.uint32), results[i].view(np.uint32)), (column, term)


# ---- 5. edges -------------------------------------------------------------------------
def test_one_world(built):
    with _sort_stress(worlds=1) as s, s.world_reduce("Item", HOLES_PLAN) as reduce:
        for step in range(3):
            _, counts, _ = _check(s, reduce, ("1 world, step", 2 * step))
            assert counts.shape == (1,) and counts[0] > 0
            s.step(2)


def test_one_world_with_many_rows(built, monkeypatch):
    """One team walks a world of more than 128 rows (the simulator's largest:
    164 rigid bodies), with 3 and with 64 lanes."""
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CANDIDATES_PER_WORLD", "4096")
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CONTACTS_PER_WORLD", "1024")
    with Simulator(hip_lib_path("ball_pit"), 1, flags=150 << 16) as s:
        dump = s.dump_all(512)
        table = max(dump, key=lambda name: int(dump[name][1].sum())).split(".", 1)[0]
        rows = int(dump[[n for n in dump if n.startswith(table + ".")][0]][1].sum())
        assert rows > 128, (table, rows)
        floats = [c[0] for c in s.columns if c[0].startswith(table + ".") and c[2]
                  and 12 <= c[1] <= 32 and c[1] % 4 == 0]
        assert len(floats) >= 2, floats
        wide = [term for name in floats[:3] for term in _all_six(name)]
        with s.world_reduce(table, [(floats[0], "sum", dict(elems=3))]) as narrow, \
                s.world_reduce(table, wide) as reduce:
            assert sum(t.elems for _, t in reduce.terms) > 32
            for step in (0, 1):
                s.step(step)
                # one world: every row of the table is world 0's
                n = len(s.dump_column_raw(_index(s, floats[0]), RAW_CAP))
                assert n == rows
                for r in (narrow, reduce):
                    _, counts, _ = _check(s, r, ("ball_pit, step", step), np.zeros(n, np.int32))
                    assert counts.tolist() == [rows]


def test_empty_table(built):
    """Scratch before the first step: zero rows, all identities, zero counts."""
    plan = [("Scratch.Key", "sum"), ("Scratch.Key", "min"), ("Scratch.Key", "max"),
            ("Scratch.Key", "min", dict(dtype="i32")), ("Scratch.Key", "max", dict(dtype="i32")),
            ("Scratch.Key", "count_nonzero", dict(alarm=True))] + \
        [("Scratch.Vec3", op, dict(alarm=op != "sum", limit=-1.0 if op == "min" else 1.0))
         for op in SIX]
    with _sort_stress() as s, s.world_reduce("Scratch", plan) as reduce:
        assert len(s.dump_column_raw(_index(s, "Scratch.Key"), RAW_CAP)) == 0
        _fill_ff(reduce)
        reduce.compute()
        results, counts, alarm = _got(reduce)
        assert not counts.any() and not alarm.any()
        identities = [0, 0xFFFFFFFF, 0, 0x7FFFFFFF, 0x80000000, 0,
                      0, 0x7F800000, 0xFF800000, 0, 0, 0]
        for i, want in enumerate(identities):
            assert results[i].shape == (33, reduce.terms[i][1].elems)
            assert (results[i].view(np.uint32) == want).all(), (i, reduce.terms[i], hex(want))
        _same((results, counts, alarm), _expected(s, reduce, np.zeros(0, np.int32)), "empty")


def test_the_pinned_column(built):
    """flags bit 6: Item.Vec3 is an exported column, which the sort keeps in place."""
    with _sort_stress(flags=64) as s, s.world_reduce("Item", _all_six("Item.Vec3")) as reduce:
        s.step(2)
        results, counts, _ = _check(s, reduce, "pinned")
        n = int(counts.sum())
        exported = s.read_tensor("item_vec3")[:n]
        world = _raw_world_ids(s)
        w = int(np.argmax(counts))
        rows = exported[world == w]
        acc = np.zeros(3, np.float32)
        for row in rows:
            acc = acc + row
        assert np.array_equal(results[0][w], acc)
        s.step(3)
        _check(s, reduce, "pinned, three steps later")


# ---- 6. outputs are rewritten in full ---------------------------------------------------
def test_outputs_are_rewritten(built):
    with _sort_stress() as s, s.world_reduce("Item", OPS_AND_DTYPES) as reduce:
        s.step(3)
        _fill_ff(reduce)
        assert reduce.alarm.cpu().numpy().tolist() == [-1] * 33
        results, counts, alarm = _check(s, reduce, "after 0xFF everywhere")
        assert (counts >= 0).all() and not alarm.any() and results[0].max() < 40 * 255


# ---- 7. step mode -----------------------------------------------------------------------
def test_step_reduce_in_the_launch_lists_and_recorded_by_an_output_ring(built):
    torch = _torch()
    K, W = 5, 33
    rt = runtime_lib()
    plan = [("Item.Vec3", "sum"), ("Item.Key", "max"), ("Item.Wide", "absmax")]
    with _sort_stress() as s, _sort_stress() as twin, \
            s.world_reduce("Item", plan) as reduce, twin.world_reduce("Item", plan) as twin_reduce, \
            s.world_view("Item", ["Item.Tag8"], max_rows=4) as view:
        names = lambda graph=0: [k["name"] for k in s.profile(1, graph=graph)]   # noqa: E731
        before = names()
        twin.step(1)        # (the profiled step)
        assert not [n for n in before if n.startswith("reduce")]

        ring = torch.zeros((K, W, 3), dtype=torch.float32, device="cuda")
        count_ring = torch.zeros((K, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        reduce.every_step()
        assert rt.mwhip_set_output_ring(s.hip_exec(), reduce.buffer_ptr(0), ring.data_ptr(),
                                        W * 3 * 4, K, RING_ON_STEP) == 0
        assert rt.mwhip_set_output_ring(s.hip_exec(), reduce.counts_ptr, count_ring.data_ptr(),
                                        W * 4, K, RING_ON_STEP) == 0
        s.step_async(K)
        want = []
        for k in range(K):
            twin.step(1)
            want.append(_check(twin, twin_reduce, ("twin", k)))
        s.sync()
        recorded, recorded_counts = ring.cpu().numpy(), count_ring.cpu().numpy()
        for k in range(K):
            assert np.array_equal(recorded_counts[k], want[k][1]), ("counts of step", k)
            assert np.array_equal(recorded[k].view(np.uint32), want[k][0][0].view(np.uint32)), \
                ("slot of step", k)
        assert not np.array_equal(recorded[K - 1], recorded[K - 2])
        # the buffers themselves hold the last step's
        _same(_got(reduce), want[K - 1], "the buffers after the last step")

        # one launch, behind every task-graph node and in front of the rings
        stats = s.profile(1)
        during = [k["name"] for k in stats]
        at = during.index("reduce:reduce")
        assert during.count("reduce:reduce") == 1
        assert during[at + 1] == "ring:ring.out", during[at:]
        assert during[:at] + during[at + 2:] == before and at == len(before) - 1
        # algo_bytes: everything written + per row counted its WorldID cell and
        # its listed elements
        counts = reduce.counts.cpu().numpy().astype(np.int64)
        written = W * (4 * 64 + 8)
        read = int(counts.sum()) * (4 + 4 * 64)
        assert stats[at]["algo_bytes"] == written + read, (stats[at], written, read)

        # behind the step views, in front of the pack node
        view.every_step()
        during = names()
        at = during.index("reduce:reduce")
        assert during[at - 1] == "view:view" and during[at + 1] == "ring:ring.out", during[at - 1:]
        packed_dst = torch.zeros((W, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        in_packed = names(s.packed_step_graph(["churn"], packed_dst.data_ptr()))
        at = in_packed.index("reduce:reduce")
        assert in_packed[at - 1] == "view:view" and in_packed[at + 1] == "pack:pack.rows" \
            and in_packed[at + 2] == "ring:ring.out", in_packed[at - 1:]
        view.every_step(False)

        for src in (reduce.buffer_ptr(0), reduce.counts_ptr):
            assert rt.mwhip_set_output_ring(s.hip_exec(), src, None, 0, 0, RING_ON_STEP) == 0
        reduce.every_step(False)
        assert names() == before

        # a ninth step reduce; destroying a step reduce unsets it
        reduces = [s.world_reduce("Item", [("Item.Key", "sum")]) for _ in range(9)]
        for r in reduces[:8]:
            r.every_step()
        launches = names()
        assert launches.count("reduce:reduce") == 1, launches
        try:
            reduces[8].every_step()
        except RuntimeError as err:
            assert "at most 8" in str(err)
        else:
            raise AssertionError("a ninth step reduce was taken")
        assert names() == launches
        reduces[0].close()
        reduces[8].every_step()
        for r in reduces[1:]:
            r.close()
        assert names() == before


# ---- 8. the guard closes the loop -------------------------------------------------------
def test_progress_of_escape_room_is_payload():
    """Agent.Progress only feeds arithmetic (rewardSystem,
    collectObservationsSystem) and a reset rewrites it."""
    src = open(os.path.join(REPO, "sims", "escape_room", "sim.cpp")).read()
    reads = [line.strip() for line in src.splitlines() if re.search(r"\bprogress\.maxY\b", line)]
    assert sorted(reads) == sorted(["float old_max_y = progress.maxY;",
                                    "progress.maxY = reward_pos;",
                                    "self_obs.maxY = progress.maxY / consts::worldLength;"]), reads
    assert "float new_progress = reward_pos - old_max_y;" in src
    assert len(re.findall(r"ctx\.get<Progress>\(agent\)\.maxY = pos\.y;", src)) >= 1
    assert not re.search(r"\[[^\]]*(old_max_y|new_progress)[^\]]*\]", src)


def test_an_alarm_resets_the_world_that_blew_up(built):
    torch = _torch()
    W, K = 16, 3
    rt = runtime_lib()
    guard = [("Agent.Progress", "count_nonfinite", dict(alarm=True))]
    with Simulator(hip_lib_path("escape_room"), W, seed=11, flags=0) as a, \
            Simulator(hip_lib_path("escape_room"), W, seed=11, flags=0) as b, \
            a.world_reduce("Agent", guard) as reduce, \
            a.world_view("Agent", ["Agent.Progress"], max_rows=4) as view, \
            a.world_write("Agent", ["Agent.Progress"], max_rows=4) as write:
        a.step(3)
        b.step(3)
        # poison one agent of world 5
        view.compute()
        assert int(view.counts.cpu().numpy()[5]) >= 2
        write.tensor("Agent.Progress").copy_(view.tensor("Agent.Progress"))
        progress = write.tensor("Agent.Progress", np.float32)
        assert tuple(progress.shape) == (W, 4, 1)
        progress[5, 1, 0] = float("inf")
        write.take.fill_(4)
        torch.cuda.synchronize()
        write.apply()
        reduce.compute()
        assert reduce.alarm.cpu().numpy().tolist() == [int(w == 5) for w in range(W)]
        reduce.alarm.zero_()
        torch.cuda.synchronize()

        alarms = torch.full((K, W), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        reduce.every_step()
        a.set_input_ring("reset", reduce.alarm_ptr, 1)
        assert rt.mwhip_set_output_ring(a.hip_exec(), reduce.alarm_ptr, alarms.data_ptr(),
                                        W * 4, K, RING_ON_STEP) == 0
        a.step_async(K)
        a.sync()

        b.step(1)
        reset = np.zeros((W, 1), np.int32)
        reset[5] = 1
        b.write_tensor("reset", reset)
        b.step(2)

        recorded = alarms.cpu().numpy()
        assert recorded[0].tolist() == [int(w == 5) for w in range(W)]
        assert not recorded[1:].any()
        assert not reduce.alarm.cpu().numpy().any()
        a.set_input_ring("reset", 0, 1)
        assert rt.mwhip_set_output_ring(a.hip_exec(), reduce.alarm_ptr, None, 0, 0,
                                        RING_ON_STEP) == 0
        got, want = a.dump_all(512), b.dump_all(512)
        assert list(got) == list(want)
        progress = got["Agent.Progress"][0].view(np.float32)
        assert np.isfinite(progress).all()
        # the reset happened
        for name in ("Agent.StepsRemaining", "Agent.Entity"):
            assert np.array_equal(got[name][0], want[name][0]), name
        for name in want:
            assert np.array_equal(got[name][1], want[name][1]), name
            assert np.array_equal(got[name][0], want[name][0]), \
                (name, "differs after a poisoned step and a reset")


# ---- 9. stream order, 10. growth, 11. restore ---------------------------------------------
def test_compute_async_is_stream_ordered(built):
    with _sort_stress() as s, _sort_stress() as twin, \
            s.world_reduce("Item", HOLES_PLAN) as reduce, \
            twin.world_reduce("Item", HOLES_PLAN) as twin_reduce:
        s.step_async(3)
        reduce.compute_async()
        s.step_async(3)
        s.sync()
        twin.step(3)
        want = _check(twin, twin_reduce, "twin, 3 steps")
        _same(_got(reduce), want, "queued between two runs of three steps")
        twin.step(3)
        later = _check(twin, twin_reduce, "twin, 6 steps")
        assert not np.array_equal(later[0][6], want[0][6])
        reduce.compute()
        _same(_got(reduce), later, "six steps")


def test_growth(built, monkeypatch):
    """The reduce is made before the tables grow."""
    monkeypatch.setenv("MADRONA_MWHIP_INITIAL_CAPACITY_DIV", "4")
    rt = runtime_lib()
    rt.mwhip_num_table_growths.restype = C.c_uint32
    rt.mwhip_num_table_growths.argtypes = [C.c_void_p]
    plan = _all_six("Item.Vec3") + [("Item.Key", "sum"), ("Item.Wide", "sum"),
                                    ("Item.Tag8", "max")]
    with _sort_stress(worlds=300, flags=2) as s, s.world_reduce("Item", plan) as reduce:
        s.step(3)
        _check(s, reduce, "before the growth")
        grown = rt.mwhip_num_table_growths(s.hip_exec())
        s.step(37)
        assert rt.mwhip_num_table_growths(s.hip_exec()) > grown, "nothing grew"
        _, counts, _ = _check(s, reduce, "after the growth")
        assert counts.max() == 40


def test_restore_then_compute_gives_the_saved_values(built):
    with _sort_stress() as s, s.world_reduce("Item", HOLES_PLAN) as reduce:
        s.step(3)
        snap = s.snapshot()
        snap.save()
        at_save = _check(s, reduce, "at the save")
        s.step(4)
        later = _check(s, reduce, "4 steps later")
        assert not np.array_equal(later[0][6], at_save[0][6])
        snap.restore()
        # (reduces are derived state: the buffers still hold the later values)
        _same(_got(reduce), later, "restored, not yet computed")
        reduce.compute()
        _same(_got(reduce), at_save, "restored and computed")
        snap.close()


# ---- 12. lock step with the reference ---------------------------------------------------
@pytest.mark.parametrize("worlds", [8, 64])
def test_lock_step_with_the_reference(built, worlds):
    """After 20 steps of escape_room_phys the HIP reduce equals reduce_ref over
    the REFERENCE backend's per-world dump."""
    _need_ref("escape_room_phys")
    physics = [(name, op) for name in ("PhysicsEntity.Position", "PhysicsEntity.Velocity")
               for op in ("sum", "absmax", "count_nonfinite")]
    agents = [(name, op) for name in ("Agent.Position", "Agent.Velocity")
              for op in ("sum", "absmax", "count_nonfinite")] + [("Agent.Reward", "sum")]
    with Simulator(ref_lib_path("escape_room_phys"), worlds, seed=5, num_workers=1) as ref, \
            Simulator(hip_lib_path("escape_room_phys"), worlds, seed=5) as hip, \
            hip.world_reduce("PhysicsEntity", physics) as phys_reduce, \
            hip.world_reduce("Agent", agents) as agent_reduce:
        rng = np.random.default_rng(worlds)
        for _ in range(20):
            shape = (worlds, 2)
            action = np.stack([rng.integers(0, 4, shape), rng.integers(0, 8, shape),
                               rng.integers(-2, 3, shape), rng.integers(0, 2, shape)],
                              -1).astype(np.int32)
            ref.write_tensor("action", action)
            hip.write_tensor("action", action)
            ref.step(1)
            hip.step(1)
        ref_names = [c[0] for c in ref.columns]
        for reduce in (phys_reduce, agent_reduce):
            reduce.compute()
            results, counts, alarm = _got(reduce)
            assert counts.min() > 0 and not alarm.any()
            for i, (column, term) in enumerate(reduce.terms):
                rows, per_world = ref.dump_column(ref_names.index(column), 512)
                want, want_counts = reduce_ref.reduce_of_dump(rows, per_world, worlds, term)
                assert np.array_equal(counts, want_counts), (column, term)
                assert np.array_equal(results[i].view(np.uint32), want.view(np.uint32)), \
                    (column, term)
            assert results[0].any()


# ---- 13. refusals -----------------------------------------------------------------------
def _ids(sim, name):
    arch, comp = C.c_uint32(0), C.c_uint32(0)
    assert sim.lib.sim_hip_column_ids(sim.handle, _index(sim, name), C.byref(arch),
                                      C.byref(comp)) == 0
    return arch.value, comp.value


def test_refusals(built):
    rt = runtime_lib()
    F32, I32, U32, U8 = 0, 1, 2, 3
    SUM, MIN, MAX, ABSMAX, NONZERO, NONFINITE = range(6)
    with _sort_stress(worlds=3) as s, _sort_stress(worlds=3) as other:
        keeper = s.world_reduce("Item", HOLES_PLAN)
        s.step(1)
        exec_ = s.hip_exec()
        item, key = _ids(s, "Item.Key")
        scratch, _ = _ids(s, "Scratch.Key")
        _, wide = _ids(s, "Item.Wide")
        _, vec3 = _ids(s, "Item.Vec3")
        _, tag8 = _ids(s, "Item.Tag8")
        _, half = _ids(s, "Item.Half")
        want = _check(s, keeper, "before the refusals")

        def create(archetype, terms, n=None):
            arr = (ReduceTerm * max(len(terms), 1))(*[ReduceTerm(*t) for t in terms])
            out = C.c_uint64(99)
            rc = rt.mwhip_reduce_create(exec_, archetype, arr, len(terms) if n is None else n,
                                        C.byref(out))
            return rc, out.value, rt.mwhip_last_error().decode()

        ok = (vec3, 0, 3, F32, SUM, 0, 0.0)
        for archetype, terms, n, word in (
                (item, [ok], 0, "n == 0"),
                (item, [ok] * 33, None, "at most 32"),
                (item, [(wide, 0, 60, F32, SUM, 0, 0.0)] * 5, None, "at most 256"),
                (item, [ok, (vec3, 0, 0, F32, SUM, 0, 0.0)], None, "term 1: num_elems == 0"),
                (item, [(vec3, 4, 3, F32, SUM, 0, 0.0)], None, "leaves the cell"),
                (item, [(vec3, 0, 13, U8, SUM, 0, 0.0)], None, "leaves the cell"),
                (item, [(tag8, 0, 1, U32, SUM, 0, 0.0)], None, "not a multiple"),
                (item, [(half, 0, 1, U32, SUM, 0, 0.0)], None, "not a multiple"),
                (item, [(vec3, 2, 1, F32, SUM, 0, 0.0)], None, "not a multiple of the element size"),
                (item, [(vec3, 0, 3, 4, SUM, 0, 0.0)], None, "unknown dtype 4"),
                (item, [(vec3, 0, 3, F32, 6, 0, 0.0)], None, "unknown op 6"),
                (item, [(vec3, 0, 3, F32, SUM, 2, 0.0)], None, "unknown flags"),
                (item, [(key, 0, 1, U32, ABSMAX, 0, 0.0)], None, "needs F32"),
                (item, [(key, 0, 1, I32, NONFINITE, 0, 0.0)], None, "needs F32"),
                (item, [(tag8, 0, 1, U8, ABSMAX, 0, 0.0)], None, "needs F32"),
                (item, [(vec3, 0, 3, F32, SUM, 1, 0.0)], None, "an alarm has no rule"),
                (item, [(key, 0, 1, U32, MAX, 1, 0.0)], None, "an alarm has no rule"),
                (item, [(key, 0, 1, I32, MIN, 1, 0.0)], None, "an alarm has no rule"),
                (250, [ok], None, "archetype 250 is not registered"),
                (scratch, [(wide, 0, 60, F32, SUM, 0, 0.0)], None,
                 "has no component %d" % wide)):
            rc, out, message = create(archetype, terms, n)
            assert rc != 0 and out == 99 and word in message, (terms[:2], rc, out, message)
            assert "reduce_create" in message, message

        # what IS allowed: a component in several terms, Entity and WorldID, alarms with a rule
        rc, handle, message = create(item, [
            ok, (vec3, 4, 2, F32, MAX, 1, 3.0), (vec3, 0, 12, U8, NONZERO, 1, 0.0),
            (0, 0, 2, U32, MAX, 0, 0.0), (1, 0, 1, I32, MIN, 0, 0.0),
            (key, 0, 1, I32, NONZERO, 1, 0.0), (vec3, 8, 1, F32, MIN, 1, 0.0),
            (vec3, 0, 3, F32, ABSMAX, 1, 1.0), (vec3, 0, 3, F32, NONFINITE, 1, 0.0)])
        assert rc == 0 and handle not in (0, 99), message
        assert rt.mwhip_reduce_compute(exec_, handle) == 0
        nbytes, elems = C.c_uint64(0), C.c_uint32(0)
        assert rt.mwhip_reduce_buffer(exec_, handle, 2, C.byref(nbytes), C.byref(elems))
        assert (nbytes.value, elems.value) == (3 * 12 * 4, 12)
        ptrs = [rt.mwhip_reduce_buffer(exec_, handle, t, None, None) for t in range(9)]
        ptrs += [rt.mwhip_reduce_counts(exec_, handle), rt.mwhip_reduce_alarm(exec_, handle)]
        assert all(p and p % 256 == 0 for p in ptrs) and len(set(ptrs)) == 11
        assert max(ptrs) - min(ptrs) < 11 * 256 + 3 * 23 * 4     # one allocation
        assert rt.mwhip_reduce_buffer(exec_, handle, 9, C.byref(nbytes), C.byref(elems)) is None
        assert "term 9 of 9" in rt.mwhip_last_error().decode()
        assert (nbytes.value, elems.value) == (3 * 12 * 4, 12)
        assert rt.mwhip_reduce_compute(other.hip_exec(), handle) != 0
        assert "reduce %d is not one of this executor's" % handle in rt.mwhip_last_error().decode()
        rt.mwhip_reduce_destroy(exec_, handle)
        for call in (lambda: rt.mwhip_reduce_compute(exec_, handle),
                     lambda: rt.mwhip_reduce_compute_async(exec_, handle),
                     lambda: rt.mwhip_set_step_reduce(exec_, handle, 1)):
            assert call() != 0
            assert "reduce %d is not one of this executor's" % handle in \
                rt.mwhip_last_error().decode()
        assert rt.mwhip_reduce_buffer(exec_, handle, 0, None, None) is None
        assert rt.mwhip_reduce_counts(exec_, handle) is None
        assert rt.mwhip_reduce_alarm(exec_, handle) is None

        # the Python wrapper refuses what it can see itself
        for bad, error in (([("Item.Nothing", "sum")], KeyError),
                           ([("Scratch.Key", "sum")], KeyError),
                           ([("Item.Key", "median")], ValueError),
                           ([("Item.Key", "sum", dict(dtype="f64"))], ValueError),
                           ([("Item.Key", "sum", dict(stride=4))], TypeError),
                           ([], ValueError)):
            with pytest.raises(error):
                s.world_reduce("Item", bad)
        with pytest.raises(RuntimeError, match="leaves the cell"):
            s.world_reduce("Item", [("Item.Vec3", "sum", dict(elems=4))])
        assert s._reduces == [keeper]

        # nothing changed for the reduce that was there all along, and the executor steps
        s.step(2)
        after = _check(s, keeper, "after the refusals")
        assert not np.array_equal(after[0][6], want[0][6])
    # Simulator.close() orphaned it
    try:
        keeper.compute()
    except RuntimeError as err:
        assert "closed" in str(err)
    else:
        raise AssertionError("a world reduce outlived its simulator")
