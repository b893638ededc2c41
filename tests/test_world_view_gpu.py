"""-m gpu: world views (mwhip_view_*, Simulator.world_view()).

The yardstick is madrona_amd/view_ref.py, the definition in numpy, evaluated
over the table-order dump (dump_column_raw): every byte of every buffer, padding
included, and every count must equal it.  Shapes are the smallest at which the
kernel can still go wrong: cells of every width it copies differently (1, 2,
4, 8, 12, 16, 20 and 240 bytes), every team size (1 .. 64 lanes per world) and
max_rows past 64, a world whose rows straddle a 256-row block, several worlds
in one wavefront, empty worlds and empty tables, truncation, holes in the
sorted prefix, rows behind it and a table with no prefix at all.
"""
import ctypes as C
import os

import numpy as np
import pytest

from madrona_amd import view_ref
from madrona_amd.simlib import (RING_ON_STEP, Simulator, hip_lib_path, ref_lib_path,
                                runtime_lib)

pytestmark = pytest.mark.gpu

CHURN_ONLY = 1      # sort_stress: churn without the compaction behind it
SORT_BY_KEY = 2     # sort_stress: a sort of Item by Key (no world-sorted prefix is left)
RAW_CAP = 1 << 16   # rows a table-order dump has room for


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


def _item_columns(sim):
    return [c[0] for c in sim.columns if c[0].startswith("Item.")]


def _raw_world_ids(sim, table="Item"):
    return sim.dump_column_raw(_index(sim, table + ".WorldID"), RAW_CAP).view(np.int32).ravel()


def _expected(sim, view, world_ids=None):
    """view_ref over the table-order dump: {column: padded}, counts"""
    if world_ids is None:
        world_ids = _raw_world_ids(sim, view.table)
    out, counts = {}, None
    for name in view.columns:
        raw = sim.dump_column_raw(_index(sim, name), RAW_CAP)
        assert len(raw) == len(world_ids), (name, len(raw), len(world_ids))
        out[name], counts = view_ref.view_of_raw(world_ids, raw, sim.num_worlds, view.max_rows)
    return out, counts


def _got(view):
    view._sim.sync()
    return ({name: view.tensor(name).cpu().numpy() for name in view.columns},
            view.counts.cpu().numpy())


def _same(got, want, what):
    got_cols, got_counts = got
    want_cols, want_counts = want
    assert got_counts.dtype == np.int32 and got_counts.shape == want_counts.shape
    bad = np.flatnonzero(got_counts != want_counts)
    assert len(bad) == 0, (what, "counts differ at worlds", bad[:4].tolist(),
                           got_counts[bad[:4]].tolist(), want_counts[bad[:4]].tolist())
    assert list(got_cols) == list(want_cols)
    for name, want_bytes in want_cols.items():
        got_bytes = got_cols[name]
        assert got_bytes.dtype == np.uint8 and got_bytes.shape == want_bytes.shape, \
            (what, name, got_bytes.shape, want_bytes.shape)
        bad = np.argwhere(got_bytes != want_bytes)
        assert len(bad) == 0, (what, name, len(bad), "bytes differ, first (world, row, byte):",
                               bad[:4].tolist())


def _check(sim, view, what, world_ids=None):
    view.compute()
    want = _expected(sim, view, world_ids)
    _same(_got(view), want, what)
    return want


# ---- 1. widths and wave shapes ------------------------------------------------------
def test_every_cell_width_and_wave_shape(built):
    with _sort_stress() as s, s.world_view("Item", max_rows=40) as view:
        assert view.columns == _item_columns(s)
        widths = sorted(view.cell_bytes(n) for n in view.columns)
        assert widths == [1, 2, 4, 4, 8, 8, 12, 16, 20, 240], widths
        straddles = three_in_a_wave = empty_world = False
        steps = 0
        for until in (0, 1, 7):
            s.step(until - steps)
            steps = until
            world = _raw_world_ids(s)
            # (after a full step the table is grouped by world, without holes)
            assert (np.diff(world) >= 0).all() and (world >= 0).all()
            _, counts = _check(s, view, ("step", until), world)
            assert counts.sum() == len(world) and counts.max() <= 40
            ends = np.cumsum(counts.astype(np.int64))
            starts = ends - counts
            straddles |= bool(((counts > 0) & (starts // 256 != (ends - 1) // 256)).any())
            three_in_a_wave |= any(len(np.unique(world[at:at + 64])) >= 3
                                   for at in range(0, len(world), 64))
            empty_world |= bool((counts == 0).any())
        assert straddles, "no world's Item rows straddle a 256-row block boundary"
        assert three_in_a_wave, "no 64-row stretch of Item holds rows of 3 worlds"
        assert empty_world, "no world without Item rows"


# ---- 2. team sizes and truncation ---------------------------------------------------
@pytest.mark.parametrize("max_rows", [1, 3, 16, 64, 100])
def test_team_sizes_and_truncation(built, max_rows):
    with _sort_stress() as s, s.world_view("Item", max_rows=max_rows) as view:
        s.step(2)
        world = _raw_world_ids(s)
        cols, counts = _check(s, view, ("max_rows", max_rows), world)
        assert cols["Item.Key"].shape == (33, max_rows, 4)
        if max_rows == 16:
            over = np.flatnonzero(counts > max_rows)
            assert len(over) != 0, "no world holds more than 16 items"
            w = int(over[0])
            rows = np.flatnonzero(world == w)[:16]
            got = view.tensor("Item.Wide").cpu().numpy()[w]
            raw = s.dump_column_raw(_index(s, "Item.Wide"), RAW_CAP)
            assert np.array_equal(got, raw[rows]), "not the first 16 rows in table order"
            assert int(view.counts.cpu().numpy()[w]) == int((world == w).sum()) > 16
        if max_rows >= 64:
            # typed tensors over the same bytes
            vec3 = view.tensor("Item.Vec3", np.float32)
            assert tuple(vec3.shape) == (33, max_rows, 3)
            assert np.array_equal(vec3.cpu().numpy().view(np.uint8).reshape(33, max_rows, 12),
                                  cols["Item.Vec3"])
            assert not cols["Item.Vec3"][:, 40:].any()


# ---- 3. padding is rewritten --------------------------------------------------------
def test_padding_is_rewritten(built):
    with _sort_stress() as s, s.world_view("Item", max_rows=40) as view:
        s.step(3)
        for name in view.columns:
            view.tensor(name).fill_(0xFF)
        view.counts.fill_(-1)
        _torch().cuda.synchronize()
        cols, counts = _check(s, view, "after 0xFF everywhere")
        assert (counts < 40).any() and (counts >= 0).all()
        # (the padding compared above is most of the buffer)
        assert sum(int((c == 0).sum()) for c in cols.values()) > 33 * 40 * 100


# ---- 4. holes and an unsorted tail --------------------------------------------------
def test_holes_and_an_unsorted_tail(built):
    with _sort_stress() as s, s.world_view("Item", max_rows=40) as view:
        s.step(4)
        saw_hole = saw_descending = False
        for rnd in range(3):
            s.run_taskgraph(CHURN_ONLY)
            world = _raw_world_ids(s)
            saw_hole |= bool((world == -1).any())
            saw_descending |= bool((np.diff(world) < 0).any())
            _check(s, view, ("churn", rnd), world)
        assert saw_hole, "no destroyed row (WorldID -1) in the raw table"
        assert saw_descending, "the raw world ids are non-decreasing"
        # no sorted prefix at all: rows of a world are scattered over the table
        s.run_taskgraph(SORT_BY_KEY)
        world = _raw_world_ids(s)
        live = world[world >= 0]
        assert (np.diff(live) < 0).sum() > len(live) // 4, "the key sort left the worlds grouped"
        _check(s, view, "sorted by key", world)
        # (this is the state dump_column refuses); after a full step both dumps agree
        s.step(1)
        cols, counts = _check(s, view, "after the next full step")
        for name in view.columns:
            rows, per_world = s.dump_column(_index(s, name), 512)
            padded, dumped_counts = view_ref.view_of_dump(rows, per_world, s.num_worlds, 40)
            assert np.array_equal(dumped_counts, counts), name
            assert np.array_equal(padded, cols[name]), name


# ---- 5. edges -----------------------------------------------------------------------
def test_one_world(built):
    with _sort_stress(worlds=1) as s, s.world_view("Item", max_rows=40) as view:
        for step in range(3):
            _, counts = _check(s, view, ("1 world, step", 2 * step))
            assert counts.shape == (1,) and counts[0] > 0
            s.step(2)


@pytest.mark.parametrize("max_rows", [256, 100])
def test_one_world_with_many_rows(built, monkeypatch, max_rows):
    """One team of 64 lanes walks a world of more than 128 rows (the simulator's
    largest: 164 rigid bodies); at 100 it drops the rest."""
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CANDIDATES_PER_WORLD", "4096")
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CONTACTS_PER_WORLD", "1024")
    with Simulator(hip_lib_path("ball_pit"), 1, flags=150 << 16) as s:
        dump = s.dump_all(512)
        table = max(dump, key=lambda name: int(dump[name][1].sum())).split(".", 1)[0]
        rows = int(dump[[n for n in dump if n.startswith(table + ".")][0]][1].sum())
        assert rows > 128, (table, rows)
        with s.world_view(table, max_rows=max_rows) as view:
            for step in (0, 1):
                s.step(step)
                # one world: every row of the table is world 0's
                n = len(s.dump_column_raw(_index(s, view.columns[0]), RAW_CAP))
                assert n == rows
                _, counts = _check(s, view, ("ball_pit, step", step), np.zeros(n, np.int32))
                assert counts.tolist() == [rows]


def test_empty_table(built):
    """Scratch before the first step: zero rows."""
    with _sort_stress() as s, s.world_view("Scratch", max_rows=8) as view:
        assert len(s.dump_column_raw(_index(s, "Scratch.Key"), RAW_CAP)) == 0
        for name in view.columns:
            view.tensor(name).fill_(0xFF)
        view.counts.fill_(7)
        _torch().cuda.synchronize()
        view.compute()
        cols, counts = _got(view)
        assert view.columns == ["Scratch.Key", "Scratch.Vec3"]
        assert not counts.any()
        assert cols["Scratch.Key"].shape == (33, 8, 4) and cols["Scratch.Vec3"].shape == (33, 8, 12)
        assert not cols["Scratch.Key"].any() and not cols["Scratch.Vec3"].any()


def test_one_one_byte_column(built):
    with _sort_stress() as s, s.world_view("Item", ["Item.Tag8"], max_rows=40) as view:
        s.step(3)
        assert view.cell_bytes("Item.Tag8") == 1
        cols, _ = _check(s, view, "one 1-byte column")
        assert list(cols) == ["Item.Tag8"] and cols["Item.Tag8"].any()


# ---- 6. lock step with the reference ------------------------------------------------
def _largest_table(sim):
    dump = sim.dump_all(512)
    name = max(dump, key=lambda n: int(dump[n][1].sum()))
    return name.split(".", 1)[0], int(dump[name][1].max())


@pytest.mark.parametrize("sim,worlds,flags", [("sort_stress", 33, 0), ("hideseek", 8, 15)])
def test_lock_step_with_the_reference(built, sim, worlds, flags):
    """Every step, the view equals the reference library's per-world
    dump_column, padded (compared from step 1 on: before the first step the
    reference's observation outputs hold whatever its allocator left there)."""
    _need_ref(sim)
    with Simulator(ref_lib_path(sim), worlds, seed=5, num_workers=1, flags=flags) as ref, \
            Simulator(hip_lib_path(sim), worlds, seed=5, flags=flags) as hip:
        table, most = ("Item", 40) if sim == "sort_stress" else _largest_table(hip)
        max_rows = most + 3
        ref_names = [c[0] for c in ref.columns]
        columns = [c[0] for c in hip.columns
                   if c[0].startswith(table + ".") and c[0] in ref_names]
        assert len(columns) >= 3, columns
        with hip.world_view(table, columns, max_rows=max_rows) as view:
            for step in range(1, 11):
                ref.step(1)
                hip.step(1)
                view.compute()
                cols, counts = _got(view)
                for name in columns:
                    rows, per_world = ref.dump_column(ref_names.index(name), 512)
                    padded, ref_counts = view_ref.view_of_dump(rows, per_world, worlds, max_rows)
                    assert np.array_equal(counts, ref_counts), (sim, step, name)
                    assert np.array_equal(cols[name], padded), (sim, step, name)
                assert counts.sum() > 0


# ---- 7. growth ----------------------------------------------------------------------
def test_growth(built, monkeypatch):
    """The view is made before the tables grow."""
    _need_ref("sort_stress")
    monkeypatch.setenv("MADRONA_MWHIP_INITIAL_CAPACITY_DIV", "4")
    rt = runtime_lib()
    rt.mwhip_num_table_growths.restype = C.c_uint32
    rt.mwhip_num_table_growths.argtypes = [C.c_void_p]
    columns = ["Item.Key", "Item.Vec3", "Item.Wide", "Item.Tag8"]
    with _sort_stress(worlds=300, flags=2) as s, \
            Simulator(ref_lib_path("sort_stress"), 300, seed=7, num_workers=1, flags=2) as ref, \
            s.world_view("Item", columns, max_rows=40) as view:
        s.step(3)
        _check(s, view, "before the growth")
        grown = rt.mwhip_num_table_growths(s.hip_exec())
        s.step(37)
        assert rt.mwhip_num_table_growths(s.hip_exec()) > grown, "nothing grew"
        cols, counts = _check(s, view, "after the growth")
        ref.step(40)
        ref_names = [c[0] for c in ref.columns]
        for name in columns:
            rows, per_world = ref.dump_column(ref_names.index(name), 512)
            padded, ref_counts = view_ref.view_of_dump(rows, per_world, 300, 40)
            assert np.array_equal(counts, ref_counts), name
            assert np.array_equal(cols[name], padded), name


# ---- 8. step view with an output ring -----------------------------------------------
def test_step_view_recorded_by_output_rings(built):
    torch = _torch()
    K, M, W = 5, 40, 33
    rt = runtime_lib()
    with _sort_stress() as s, _sort_stress() as twin, \
            s.world_view("Item", ["Item.Vec3", "Item.Tag8"], max_rows=M) as view, \
            twin.world_view("Item", ["Item.Vec3", "Item.Tag8"], max_rows=M) as twin_view:
        names = lambda: [k["name"] for k in s.profile(1)]   # noqa: E731
        before = names()
        twin.step(1)        # (the profiled step)
        assert not [n for n in before if n.startswith("view")]

        ring = torch.zeros((K, W, M, 12), dtype=torch.uint8, device="cuda")
        count_ring = torch.zeros((K, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        view.every_step()
        assert rt.mwhip_set_output_ring(s.hip_exec(), view.buffer_ptr("Item.Vec3"),
                                        ring.data_ptr(), W * M * 12, K, RING_ON_STEP) == 0
        assert rt.mwhip_set_output_ring(s.hip_exec(), view.counts_ptr, count_ring.data_ptr(),
                                        W * 4, K, RING_ON_STEP) == 0
        s.step_async(K)
        want = []
        for k in range(K):
            twin.step(1)
            want.append(_check(twin, twin_view, ("twin", k)))
        s.sync()
        recorded, recorded_counts = ring.cpu().numpy(), count_ring.cpu().numpy()
        for k in range(K):
            assert np.array_equal(recorded_counts[k], want[k][1]), ("counts of step", k)
            assert np.array_equal(recorded[k], want[k][0]["Item.Vec3"]), ("slot of step", k)
        assert not np.array_equal(recorded[K - 1], recorded[K - 2])
        # the buffers themselves hold the last step's
        _same(_got(view), want[K - 1], "the buffers after the last step")

        # one launch, behind every task-graph node and in front of the rings
        stats = s.profile(1)
        during = [k["name"] for k in stats]
        at = during.index("view:view")
        assert during.count("view:view") == 1
        assert during[at + 1] == "ring:ring.out", during[at:]
        assert during[:at] + during[at + 2:] == before and at == len(before) - 1
        # algo_bytes: everything written + the cells copied + the WorldID cells read
        counts = view.counts.cpu().numpy().astype(np.int64)
        written = W * M * 13 + W * 4
        read = int(np.minimum(counts, M).sum()) * 13 + int(counts.sum()) * 4
        assert stats[at]["algo_bytes"] == written + read, (stats[at], written, read)

        for src in (view.buffer_ptr("Item.Vec3"), view.counts_ptr):
            assert rt.mwhip_set_output_ring(s.hip_exec(), src, None, 0, 0, RING_ON_STEP) == 0
        view.every_step(False)
        assert names() == before


# ---- 9. stream order and restore ----------------------------------------------------
def test_compute_async_is_stream_ordered(built):
    with _sort_stress() as s, _sort_stress() as twin, \
            s.world_view("Item", max_rows=40) as view, \
            twin.world_view("Item", max_rows=40) as twin_view:
        s.step_async(3)
        view.compute_async()
        s.step_async(3)
        s.sync()
        twin.step(3)
        want = _check(twin, twin_view, "twin, 3 steps")
        _same(_got(view), want, "queued between two runs of three steps")
        twin.step(3)
        later = _check(twin, twin_view, "twin, 6 steps")
        assert not np.array_equal(later[0]["Item.Key"], want[0]["Item.Key"])
        view.compute()
        _same(_got(view), later, "six steps")


def test_restore_then_compute_gives_the_saved_view(built):
    with _sort_stress() as s, s.world_view("Item", max_rows=40) as view:
        s.step(3)
        snap = s.snapshot()
        snap.save()
        at_save = _check(s, view, "at the save")
        s.step(4)
        later = _check(s, view, "4 steps later")
        assert not np.array_equal(later[0]["Item.Key"], at_save[0]["Item.Key"])
        snap.restore()
        # (views are derived state: the buffers still hold the later view)
        _same(_got(view), later, "restored, not yet computed")
        view.compute()
        _same(_got(view), at_save, "restored and computed")
        snap.close()


# ---- 10. refusals at the ABI --------------------------------------------------------
def _ids(sim, name):
    arch, comp = C.c_uint32(0), C.c_uint32(0)
    assert sim.lib.sim_hip_column_ids(sim.handle, _index(sim, name), C.byref(arch),
                                      C.byref(comp)) == 0
    return arch.value, comp.value


def test_refusals(built):
    rt = runtime_lib()
    with _sort_stress(worlds=3) as s, _sort_stress(worlds=3) as other:
        keeper = s.world_view("Item", max_rows=40)
        s.step(1)
        exec_ = s.hip_exec()
        item, key = _ids(s, "Item.Key")
        scratch, _ = _ids(s, "Scratch.Key")
        _, wide = _ids(s, "Item.Wide")
        want = _check(s, keeper, "before the refusals")

        def create(archetype, comps, max_rows, n=None):
            arr = (C.c_uint32 * max(len(comps), 1))(*comps)
            out = C.c_uint64(99)
            rc = rt.mwhip_view_create(exec_, archetype, arr, len(comps) if n is None else n,
                                      max_rows, C.byref(out))
            return rc, out.value, rt.mwhip_last_error().decode()

        for archetype, comps, max_rows, n, word in (
                (item, [key], 4, 0, "n == 0"),
                (item, [key] * 33, 4, None, "at most 32"),
                (item, [key], 0, None, "max_rows == 0"),
                (250, [key], 4, None, "archetype 250 is not registered"),
                (scratch, [wide], 4, None, "has no component %d" % wide),
                (item, [key, 1, key], 4, None, "component %d is listed twice" % key),
                # 3 worlds x 2^32 - 1 rows x 240 bytes: more than any device has
                (item, [wide], 0xFFFFFFFF, None, "no device memory")):
            rc, out, message = create(archetype, comps, max_rows, n)
            assert rc != 0 and out == 99 and word in message, (comps[:3], rc, out, message)

        # handles: unknown, destroyed, another executor's
        rc, handle, message = create(item, [key, 1, 0], 4)
        assert rc == 0 and handle not in (0, 99), message
        assert rt.mwhip_view_compute(exec_, handle) == 0
        nbytes, cell = C.c_uint64(0), C.c_uint32(0)
        assert rt.mwhip_view_buffer(exec_, handle, 2, C.byref(nbytes), C.byref(cell))
        assert (nbytes.value, cell.value) == (3 * 4 * 8, 8)
        assert rt.mwhip_view_buffer(exec_, handle, 3, C.byref(nbytes), C.byref(cell)) is None
        assert "column 3 of 3" in rt.mwhip_last_error().decode()
        assert (nbytes.value, cell.value) == (3 * 4 * 8, 8)
        assert rt.mwhip_view_compute(other.hip_exec(), handle) != 0
        assert "view %d is not one of this executor's" % handle in rt.mwhip_last_error().decode()
        rt.mwhip_view_destroy(exec_, handle)
        for call in (lambda: rt.mwhip_view_compute(exec_, handle),
                     lambda: rt.mwhip_view_compute_async(exec_, handle),
                     lambda: rt.mwhip_set_step_view(exec_, handle, 1)):
            assert call() != 0
            assert "view %d is not one of this executor's" % handle in \
                rt.mwhip_last_error().decode()
        assert rt.mwhip_view_buffer(exec_, handle, 0, None, None) is None
        assert rt.mwhip_view_counts(exec_, handle) is None

        # a ninth step view; destroying a step view unsets it
        views = [s.world_view("Item", ["Item.Key"], max_rows=2) for _ in range(9)]
        for v in views[:8]:
            v.every_step()
        launches = [k["name"] for k in s.profile(1)]
        assert launches.count("view:view") == 1, launches
        try:
            views[8].every_step()
        except RuntimeError as err:
            assert "at most 8" in str(err)
        else:
            raise AssertionError("a ninth step view was taken")
        views[0].close()
        views[8].every_step()
        for v in views[1:]:
            v.close()
        assert "view:view" not in [k["name"] for k in s.profile(1)]

        # nothing changed for the view that was there all along, and the executor steps
        s.step(2)
        after = _check(s, keeper, "after the refusals")
        assert not np.array_equal(after[0]["Item.Key"], want[0]["Item.Key"])
    # Simulator.close() orphaned it
    try:
        keeper.compute()
    except RuntimeError as err:
        assert "closed" in str(err)
    else:
        raise AssertionError("a world view outlived its simulator")
