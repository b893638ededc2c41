"""-m gpu: world writes (mwhip_write_*, Simulator.world_write()).

The yardstick is madrona_amd/write_ref.py, the definition in numpy, evaluated
over the table-order dump (dump_column_raw) taken before the apply: after it,
every byte of every column of the table -- the listed ones, the unlisted ones,
Entity and WorldID -- and every count must equal it.  Shapes are those at which
the view tests established their preconditions (sort_stress, 33 worlds, seed 7,
the Item table: cells of 1, 2, 4, 4, 8, 8, 12, 16, 20 and 240 bytes, of which a
write may list all but Entity's 8 and WorldID's 4): every team size and
max_rows past 64, a world whose rows straddle a 256-row block, several worlds
in one wavefront, empty worlds and tables, truncation, holes in the sorted
prefix, rows behind it and a table with no prefix at all.
"""
import ctypes as C
import os

import numpy as np
import pytest

from madrona_amd import view_ref, write_ref
from madrona_amd.simlib import (RING_ON_STEP, Simulator, hip_lib_path, ref_lib_path,
                                runtime_lib)

pytestmark = pytest.mark.gpu

CHURN_ONLY = 1      # sort_stress: churn without the compaction behind it
SORT_BY_KEY = 2     # sort_stress: a sort of Item by Key (no world-sorted prefix is left)
RAW_CAP = 1 << 16   # rows a table-order dump has room for
ITEM_WIDTHS = [1, 2, 4, 4, 8, 8, 12, 16, 20, 240]     # Entity and WorldID included
WRITABLE_WIDTHS = [1, 2, 4, 8, 12, 16, 20, 240]


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


def _table_columns(sim, table):
    return [c[0] for c in sim.columns if c[0].startswith(table + ".")]


def _dump_table(sim, table="Item"):
    """{column: uint8 [rows, cell]} of EVERY dump-list column of the table, in
    table order, destroyed rows included"""
    return {name: sim.dump_column_raw(_index(sim, name), RAW_CAP)
            for name in _table_columns(sim, table)}


def _world_ids(dump, table="Item"):
    return dump[table + ".WorldID"].view(np.int32).ravel()


def _fill(write, rng, take):
    """Seeded random bytes into every slab, `take` into take; returns the slabs"""
    torch = _torch()
    slabs = {}
    for name in write.columns:
        slabs[name] = rng.integers(0, 256, (write.num_worlds, write.max_rows,
                                            write.cell_bytes(name))).astype(np.uint8)
        write.tensor(name).copy_(torch.from_numpy(slabs[name]).cuda())
    write.take.copy_(torch.from_numpy(np.asarray(take, np.int32)).cuda())
    # (torch's stream against the executor's: the caller's to order)
    torch.cuda.synchronize()
    return slabs


def _random_take(rng, worlds, max_rows):
    return rng.integers(-2, max_rows + 4, worlds).astype(np.int32)


def _same_table(got, want, what):
    assert list(got) == list(want)
    for name in want:
        assert got[name].shape == want[name].shape, (what, name, got[name].shape,
                                                     want[name].shape)
        bad = np.argwhere(got[name] != want[name])
        assert len(bad) == 0, (what, name, len(bad), "bytes differ, first (row, byte):",
                               bad[:4].tolist())


def _expected(before, world_ids, write, slabs, take):
    want, counts = dict(before), None
    for name in write.columns:
        want[name], counts = write_ref.write_of_raw(world_ids, before[name], slabs[name], take,
                                                    write.num_worlds, write.max_rows)
    return want, counts


def _apply_and_check(sim, write, slabs, take, what, world_ids=None, before=None):
    """The core check: dump, apply, dump, compare every byte of every column
    with write_ref over the first dump, and counts with its counts.  Returns
    (before, after, counts)."""
    if before is None:
        before = _dump_table(sim, write.table)
    if world_ids is None:
        world_ids = _world_ids(before, write.table)
    for name, raw in before.items():
        assert len(raw) == len(world_ids), (name, len(raw), len(world_ids))
    write.apply()
    sim.sync()
    after = _dump_table(sim, write.table)
    want, want_counts = _expected(before, world_ids, write, slabs, take)
    _same_table(after, want, what)
    counts = write.counts.cpu().numpy()
    assert counts.dtype == np.int32 and np.array_equal(counts, want_counts), \
        (what, counts.tolist(), want_counts.tolist())
    # the inputs are not modified
    assert np.array_equal(write.take.cpu().numpy(), np.asarray(take, np.int32)), what
    for name in write.columns:
        assert np.array_equal(write.tensor(name).cpu().numpy(), slabs[name]), (what, name)
    return before, after, counts


# ---- 1. widths and wave shapes ------------------------------------------------------
def test_every_cell_width_and_wave_shape(built):
    rng = np.random.default_rng(101)
    with _sort_stress() as s, s.world_write("Item", max_rows=40) as write:
        assert sorted(c[1] for c in s.columns if c[0].startswith("Item.")) == ITEM_WIDTHS
        assert write.columns == [n for n in _table_columns(s, "Item")
                                 if n not in ("Item.Entity", "Item.WorldID")]
        assert sorted(write.cell_bytes(n) for n in write.columns) == WRITABLE_WIDTHS
        # all zero at creation: an apply before anything is filled writes nothing
        zeros = {n: np.zeros((33, 40, write.cell_bytes(n)), np.uint8) for n in write.columns}
        before, after, _ = _apply_and_check(s, write, zeros, np.zeros(33, np.int32), "unfilled")
        _same_table(after, before, "unfilled")

        straddles = three_in_a_wave = empty_world = False
        steps = 0
        for until in (0, 1, 7):
            s.step(until - steps)
            steps = until
            before = _dump_table(s)
            world = _world_ids(before)
            # (after a full step the table is grouped by world, without holes)
            assert (np.diff(world) >= 0).all() and (world >= 0).all()
            table_counts = np.bincount(world, minlength=33)
            assert table_counts.max() <= 40
            take = _random_take(rng, 33, 40)
            assert take.min() >= -2 and take.max() <= 43
            # at least one world at 0, one negative, one above its count
            take[int(rng.integers(0, 11))] = 0
            take[int(rng.integers(11, 22))] = -1 - int(rng.integers(0, 2))
            take[int(rng.integers(22, 33))] = 43
            assert (take == 0).any() and (take < 0).any() and (take > table_counts).any()
            slabs = _fill(write, rng, take)
            _, after, counts = _apply_and_check(s, write, slabs, take, ("step", until),
                                                world, before)
            assert counts.sum() == len(world)
            assert any((after[n] != before[n]).any() for n in write.columns)
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
    rng = np.random.default_rng(200 + max_rows)
    with _sort_stress() as s, s.world_write("Item", max_rows=max_rows) as write:
        s.step(2)
        before = _dump_table(s)
        world = _world_ids(before)
        table_counts = np.bincount(world, minlength=33)
        take = _random_take(rng, 33, max_rows)
        over = np.flatnonzero(table_counts > max_rows)
        if max_rows == 16:
            assert len(over) != 0, "no world holds more than 16 items"
            take[over[0]] = 19      # (more than max_rows of a world that has more)
        slabs = _fill(write, rng, take)
        assert write.tensor("Item.Key").shape == (33, max_rows, 4)
        _, after, counts = _apply_and_check(s, write, slabs, take, ("max_rows", max_rows),
                                            world, before)
        assert np.array_equal(counts, table_counts)
        if max_rows == 16:
            w = int(over[0])
            rows = np.flatnonzero(world == w)
            assert len(rows) > 16 and counts[w] == len(rows)
            for name in _table_columns(s, "Item"):
                # the rows of that world from the 17th on: byte for byte what they were
                assert np.array_equal(after[name][rows[16:]], before[name][rows[16:]]), name
            assert np.array_equal(after["Item.Wide"][rows[:16]], slabs["Item.Wide"][w])
        if max_rows >= 64:
            # typed tensors over the same bytes
            vec3 = write.tensor("Item.Vec3", np.float32)
            assert tuple(vec3.shape) == (33, max_rows, 3)
            assert np.array_equal(vec3.cpu().numpy().view(np.uint8).reshape(33, max_rows, 12),
                                  slabs["Item.Vec3"])


# ---- 3. holes, a tail, no prefix ----------------------------------------------------
def test_holes_a_tail_and_no_prefix(built):
    rng = np.random.default_rng(300)
    with _sort_stress() as s, s.world_write("Item", max_rows=40) as write:
        s.step(4)
        saw_hole = saw_descending = False

        def check(what):
            before = _dump_table(s)
            world = _world_ids(before)
            take = _random_take(rng, 33, 40)
            slabs = _fill(write, rng, take)
            _, after, _ = _apply_and_check(s, write, slabs, take, what, world, before)
            dead = np.flatnonzero(world == -1)
            for name in before:
                # destroyed rows are unchanged in every column
                assert np.array_equal(after[name][dead], before[name][dead]), (what, name)
            assert any((after[n] != before[n]).any() for n in write.columns), what
            return world

        for rnd in range(3):
            s.run_taskgraph(CHURN_ONLY)
            world = check(("churn", rnd))
            saw_hole |= bool((world == -1).any())
            saw_descending |= bool((np.diff(world) < 0).any())
        assert saw_hole, "no destroyed row (WorldID -1) in the raw table"
        assert saw_descending, "the raw world ids are non-decreasing"
        # no sorted prefix at all: rows of a world are scattered over the table
        # (Key holds random bytes by now: any order will do)
        s.run_taskgraph(SORT_BY_KEY)
        world = check("sorted by key")
        live = world[world >= 0]
        assert (np.diff(live) < 0).sum() > len(live) // 4, "the key sort left the worlds grouped"
        # the simulator goes on from what was written
        s.step(1)
        check("after the next full step")


# ---- 4. edges -----------------------------------------------------------------------
def test_one_world(built):
    rng = np.random.default_rng(400)
    with _sort_stress(worlds=1) as s, s.world_write("Item", max_rows=40) as write:
        for step in range(3):
            take = np.array([(40, 3, -1)[step]], np.int32)
            slabs = _fill(write, rng, take)
            _, _, counts = _apply_and_check(s, write, slabs, take, ("1 world, step", 2 * step))
            assert counts.shape == (1,) and counts[0] > 0
            s.step(2)


@pytest.mark.parametrize("max_rows", [256, 100])
def test_one_world_with_many_rows(built, monkeypatch, max_rows):
    """One team of 64 lanes writes a world of more than 128 rows (the simulator's
    largest: 164 rigid bodies); at 100 it leaves the rest.  (Nothing is stepped
    after random bytes went into rigid-body state.)"""
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CANDIDATES_PER_WORLD", "4096")
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CONTACTS_PER_WORLD", "1024")
    rng = np.random.default_rng(410 + max_rows)
    with Simulator(hip_lib_path("ball_pit"), 1, flags=150 << 16) as s:
        s.step(1)
        dump = s.dump_all(512)
        table = max(dump, key=lambda name: int(dump[name][1].sum())).split(".", 1)[0]
        rows = int(dump[[n for n in dump if n.startswith(table + ".")][0]][1].sum())
        assert rows > 128, (table, rows)
        with s.world_write(table, max_rows=max_rows) as write:
            assert len(write.columns) >= 3, write.columns
            take = np.array([max_rows], np.int32)
            slabs = _fill(write, rng, take)
            # one world: every row of the table is world 0's
            before = _dump_table(s, table)
            n = len(before[write.columns[0]])
            assert n == rows
            _, after, counts = _apply_and_check(s, write, slabs, take, "ball_pit",
                                                np.zeros(n, np.int32), before)
            assert counts.tolist() == [rows]
            k = min(rows, max_rows)
            name = write.columns[0]
            assert np.array_equal(after[name][:k], slabs[name][0, :k])
            assert np.array_equal(after[name][k:], before[name][k:])


def test_empty_table(built):
    """Scratch before the first step: zero rows, and zero rows after."""
    rng = np.random.default_rng(420)
    with _sort_stress() as s, s.world_write("Scratch", max_rows=8) as write:
        assert write.columns == ["Scratch.Key", "Scratch.Vec3"]
        assert len(s.dump_column_raw(_index(s, "Scratch.Key"), RAW_CAP)) == 0
        write.counts.fill_(7)
        take = np.full(33, 8, np.int32)
        slabs = _fill(write, rng, take)
        _, after, counts = _apply_and_check(s, write, slabs, take, "empty table",
                                            np.zeros(0, np.int32))
        assert not counts.any()
        assert all(len(raw) == 0 for raw in after.values())
        s.step(2)       # (the table fills; the executor is as it was)
        assert len(s.dump_column_raw(_index(s, "Scratch.Key"), RAW_CAP)) > 0


def test_one_one_byte_column(built):
    rng = np.random.default_rng(430)
    with _sort_stress() as s, s.world_write("Item", ["Item.Tag8"], max_rows=40) as write:
        s.step(3)
        assert write.columns == ["Item.Tag8"] and write.cell_bytes("Item.Tag8") == 1
        take = _random_take(rng, 33, 40)
        slabs = _fill(write, rng, take)
        before, after, _ = _apply_and_check(s, write, slabs, take, "one 1-byte column")
        assert (after["Item.Tag8"] != before["Item.Tag8"]).any()


def test_the_pinned_column(built):
    """flags bit 6: Item.Vec3 is an exported column, which the sort keeps in
    place; the exported tensor shows the written bytes."""
    rng = np.random.default_rng(440)
    with _sort_stress(flags=64) as s, s.world_write("Item", ["Item.Vec3"], max_rows=40) as write:
        s.step(2)
        pin_ptr = s.tensor_ptr("item_vec3")
        take = np.full(33, 40, np.int32)
        slabs = _fill(write, rng, take)
        before, after, counts = _apply_and_check(s, write, slabs, take, "pinned")
        n = len(after["Item.Vec3"])
        assert s.tensor_ptr("item_vec3") == pin_ptr
        exported = s.read_tensor("item_vec3")[:n]
        assert np.array_equal(exported.view(np.uint8).reshape(n, 12), after["Item.Vec3"])
        world = _world_ids(before)
        w = int(np.argmax(counts))
        assert np.array_equal(exported.view(np.uint8).reshape(n, 12)[world == w],
                              slabs["Item.Vec3"][w, :counts[w]])


# ---- 5. round trip and continuation -------------------------------------------------
def test_a_view_written_back_changes_nothing(built):
    torch = _torch()
    with _sort_stress() as s, _sort_stress() as twin, \
            s.world_write("Item", max_rows=40) as write, \
            s.world_view("Item", write.columns, max_rows=40) as view, \
            s.digest() as digest:
        s.step(3)
        twin.step(3)
        before = _dump_table(s)
        digest_before = digest.compute().copy()
        view.compute()
        for name in write.columns:
            # the layouts are the same: tensor for tensor
            assert write.tensor(name).shape == view.tensor(name).shape
            write.tensor(name).copy_(view.tensor(name))
        write.take.fill_(write.max_rows)
        torch.cuda.synchronize()
        write.apply()
        _same_table(_dump_table(s), before, "a view written back")
        assert np.array_equal(write.counts.cpu().numpy(), view.counts.cpu().numpy())
        assert np.array_equal(digest.compute(), digest_before)
        _same_table(_dump_table(twin), before, "the twin")
        for step in range(5):
            s.step(1)
            twin.step(1)
            _same_table(_dump_table(s), _dump_table(twin), ("continuation, step", step))
            for table in ("Scratch",):
                _same_table(_dump_table(s, table), _dump_table(twin, table), (table, step))


# ---- 6. restore, perturb, roll out --------------------------------------------------
def test_restore_perturb_roll_out(built):
    torch = _torch()
    worlds, steps, moved = 8, 8, [1, 5]
    others = [w for w in range(worlds) if w not in moved]
    with Simulator(hip_lib_path("escape_room_phys"), worlds, seed=5, flags=15) as s, \
            s.digest() as digest, s.snapshot() as snap:
        assert "PhysicsEntity.Position" in [c[0] for c in s.columns]
        s.step(10)
        snap.save()
        first = []
        for _ in range(steps):
            s.step(1)
            first.append(digest.compute().copy())
        snap.restore()
        at_restore = digest.compute().copy()

        rows = int(s.dump_column(_index(s, "PhysicsEntity.Position"), 512)[1].max())
        with s.world_view("PhysicsEntity", ["PhysicsEntity.Position"], max_rows=rows + 2) as view, \
                s.world_write("PhysicsEntity", ["PhysicsEntity.Position"],
                              max_rows=rows + 2) as write:
            view.compute()
            counts = view.counts.cpu().numpy()
            assert counts[moved].min() > 0 and counts.max() <= write.max_rows
            write.tensor("PhysicsEntity.Position").copy_(view.tensor("PhysicsEntity.Position"))
            write.tensor("PhysicsEntity.Position", np.float32)[moved, :, 0] += 0.25
            take = torch.zeros(worlds, dtype=torch.int32, device="cuda")
            take[moved] = write.max_rows
            write.take.copy_(take)
            torch.cuda.synchronize()
            write.apply()
            assert np.array_equal(write.counts.cpu().numpy(), counts)

        after_apply = digest.compute().copy()
        # Position is in the digest: the two worlds differ right after the apply ...
        groups = [g for g, table in enumerate(digest.groups) if table == "PhysicsEntity"]
        assert len(groups) == 1
        for w in moved:
            assert after_apply[groups[0], w] != at_restore[groups[0], w], w
        # ... and the other six are what they were
        assert np.array_equal(after_apply[:, others], at_restore[:, others])
        for k in range(steps):
            s.step(1)
            now = digest.compute()
            assert np.array_equal(now[:, others], first[k][:, others]), ("step", k)
            if k == 0:
                for w in moved:
                    assert (now[:, w] != first[k][:, w]).any(), w


# ---- 7. against the reference backend -----------------------------------------------
def _largest_table(sim):
    dump = sim.dump_all(512)
    name = max(dump, key=lambda n: int(dump[n][1].sum()))
    return name.split(".", 1)[0], int(dump[name][1].max())


@pytest.mark.parametrize("sim,worlds,flags", [("sort_stress", 33, 0), ("hideseek", 8, 15)])
def test_writing_back_the_references_column(built, sim, worlds, flags):
    """Three steps in lock step, one column of the HIP side overwritten with
    0xFF and then with the reference's per-world dump of it, five more steps in
    lock step, bit for bit."""
    _need_ref(sim)
    torch = _torch()
    with Simulator(ref_lib_path(sim), worlds, seed=5, num_workers=1, flags=flags) as ref, \
            Simulator(hip_lib_path(sim), worlds, seed=5, flags=flags) as hip:
        ref.step(3)
        hip.step(3)
        table, most = ("Item", 40) if sim == "sort_stress" else _largest_table(hip)
        max_rows = most + 3
        ref_names = [c[0] for c in ref.columns]
        columns = [c[0] for c in hip.columns
                   if c[0].startswith(table + ".") and c[0] in ref_names]
        writable = [n for n in columns if n.split(".", 1)[1] not in ("Entity", "WorldID")]
        assert len(writable) >= 2, columns
        name = "Item.Key" if sim == "sort_stress" else writable[0]

        def lock_step(what):
            for col in columns:
                ref_rows, ref_counts = ref.dump_column(ref_names.index(col), 512)
                hip_rows, hip_counts = hip.dump_column(_index(hip, col), 512)
                assert np.array_equal(ref_counts, hip_counts), (sim, what, col)
                assert np.array_equal(ref_rows, hip_rows), (sim, what, col)

        lock_step("before")
        with hip.world_write(table, [name], max_rows=max_rows) as write:
            rows, per_world = ref.dump_column(ref_names.index(name), 512)
            assert per_world.max() <= max_rows and per_world.sum() > 0
            write.tensor(name).fill_(0xFF)
            write.take.fill_(max_rows)
            torch.cuda.synchronize()
            write.apply()
            spoiled, _ = hip.dump_column(_index(hip, name), 512)
            assert (spoiled == 0xFF).all() and len(spoiled) == len(rows)
            assert np.array_equal(write.counts.cpu().numpy(), per_world)
            slab, _ = view_ref.view_of_dump(rows, per_world, worlds, max_rows)
            write.tensor(name).copy_(torch.from_numpy(slab).cuda())
            torch.cuda.synchronize()
            write.apply()
        lock_step("written back")
        for step in range(5):
            ref.step(1)
            hip.step(1)
            lock_step(("step", step))


# ---- 8. step writes -----------------------------------------------------------------
def test_the_step_write_launch(built):
    """One launch, directly behind the input rings (first without one) and in
    front of the first node; gone, name for name, when unset."""
    torch = _torch()
    rng = np.random.default_rng(800)
    W, M = 33, 40
    with _sort_stress() as s, s.world_write("Item", ["Item.Key", "Item.Vec3"],
                                            max_rows=M) as write:
        s.step(2)
        names = lambda: [k["name"] for k in s.profile(1)]   # noqa: E731
        before = names()
        assert not [n for n in before if n.startswith("write") or n.startswith("input")]

        take = _random_take(rng, W, M)
        _fill(write, rng, take)
        write.every_step()
        stats = s.profile(1)
        during = [k["name"] for k in stats]
        assert during[0] == "write:write" and during[1:] == before, during
        # algo_bytes: rows written x listed row bytes x 2 + 4 bytes per WorldID cell counted
        counts = write.counts.cpu().numpy().astype(np.int64)
        written = int(np.minimum(np.minimum(np.maximum(take, 0), counts), M).sum())
        assert written > 0
        assert stats[0]["algo_bytes"] == written * 16 * 2 + int(counts.sum()) * 4, \
            (stats[0], written, int(counts.sum()))

        ring = torch.from_numpy(rng.integers(0, 256, (2, W, M, 4)).astype(np.uint8)).cuda()
        torch.cuda.synchronize()
        rt = runtime_lib()
        assert rt.mwhip_set_input_ring(s.hip_exec(), write.buffer_ptr("Item.Key"),
                                       ring.data_ptr(), W * M * 4, 2) == 0
        during = names()
        assert during[:2] == ["input:ring", "write:write"] and during[2:] == before, during
        assert during.count("write:write") == 1

        write.every_step(False)
        assert names() == ["input:ring"] + before
        assert rt.mwhip_set_input_ring(s.hip_exec(), write.buffer_ptr("Item.Key"), None,
                                       0, 0) == 0
        assert names() == before


def test_an_input_ring_feeds_the_step_write(built):
    """K queued steps carry K different injections: a 4-slot input ring feeds
    the slab of a 4-byte column, and the digest trail an output ring records
    equals that of a twin that applies the four slabs by hand between four
    single steps."""
    torch = _torch()
    rng = np.random.default_rng(810)
    K, W, M = 4, 33, 40
    rt = runtime_lib()
    with _sort_stress() as s, _sort_stress() as twin, \
            s.world_write("Item", ["Item.Key"], max_rows=M) as write, \
            twin.world_write("Item", ["Item.Key"], max_rows=M) as twin_write, \
            s.digest() as digest, twin.digest() as twin_digest:
        assert write.cell_bytes("Item.Key") == 4
        s.step(2)
        twin.step(2)
        slabs = rng.integers(0, 256, (K, W, M, 4)).astype(np.uint8)
        ring = torch.from_numpy(slabs).cuda()
        groups = len(digest.groups)
        trail = torch.zeros((K, groups, W), dtype=torch.int64, device="cuda")
        write.take.fill_(M)
        twin_write.take.fill_(M)
        torch.cuda.synchronize()

        write.every_step()
        digest.every_step()
        assert rt.mwhip_set_output_ring(s.hip_exec(), digest.buffer_ptr, trail.data_ptr(),
                                        groups * W * 8, K, RING_ON_STEP) == 0
        assert rt.mwhip_set_input_ring(s.hip_exec(), write.buffer_ptr("Item.Key"),
                                       ring.data_ptr(), W * M * 4, K) == 0
        s.step_async(K)

        want = []
        for k in range(K):
            twin_write.tensor("Item.Key").copy_(torch.from_numpy(slabs[k]).cuda())
            torch.cuda.synchronize()
            twin_write.apply()
            twin.step(1)
            want.append(twin_digest.compute().copy())
        s.sync()
        recorded = trail.cpu().numpy().view(np.uint64)
        for k in range(K):
            assert np.array_equal(recorded[k], want[k]), ("digest of step", k)
        assert not np.array_equal(recorded[K - 1], recorded[K - 2])
        # the slab holds the last slot, and the tables agree
        assert np.array_equal(write.tensor("Item.Key").cpu().numpy(), slabs[K - 1])
        _same_table(_dump_table(s), _dump_table(twin), "after the K steps")

        assert rt.mwhip_set_input_ring(s.hip_exec(), write.buffer_ptr("Item.Key"), None,
                                       0, 0) == 0
        assert rt.mwhip_set_output_ring(s.hip_exec(), digest.buffer_ptr, None, 0, 0,
                                        RING_ON_STEP) == 0


def test_a_ninth_step_write_and_destroying_a_set_one(built):
    with _sort_stress(worlds=3) as s:
        s.step(1)
        before = [k["name"] for k in s.profile(1)]
        writes = [s.world_write("Item", ["Item.Key"], max_rows=2) for _ in range(9)]
        for w in writes[:8]:
            w.every_step()
        launches = [k["name"] for k in s.profile(1)]
        assert launches.count("write:write") == 1 and launches[0] == "write:write", launches
        try:
            writes[8].every_step()
        except RuntimeError as err:
            assert "at most 8" in str(err) and "set_step_write" in str(err)
        else:
            raise AssertionError("a ninth step write was taken")
        assert [k["name"] for k in s.profile(1)] == launches
        # destroying a set write unsets it: the graphs stay runnable
        writes[0].close()
        writes[8].every_step()
        s.step(2)
        assert [k["name"] for k in s.profile(1)] == launches
        for w in writes[1:]:
            w.close()
        assert [k["name"] for k in s.profile(1)] == before
        s.step(2)
        s.step_async(2)
        s.sync()


# ---- 9. stream order ----------------------------------------------------------------
def test_apply_async_is_stream_ordered(built):
    rng = np.random.default_rng(900)
    with _sort_stress() as s, _sort_stress() as twin, \
            s.world_write("Item", max_rows=40) as write, \
            twin.world_write("Item", max_rows=40) as twin_write:
        take = _random_take(rng, 33, 40)
        slabs = _fill(write, np.random.default_rng(901), take)
        _fill(twin_write, np.random.default_rng(901), take)
        start = _dump_table(s)
        s.step_async(3)
        write.apply_async()
        s.sync()
        twin.step(3)
        twin.sync()
        before = _dump_table(twin)
        _, after, _ = _apply_and_check(twin, twin_write, slabs, take, "twin", before=before)
        _same_table(_dump_table(s), after, "step_async(3), apply_async(), sync()")
        assert np.array_equal(write.counts.cpu().numpy(), twin_write.counts.cpu().numpy())
        # (applied to the table of three steps later, not to the one it was queued at)
        assert len(start["Item.Key"]) != len(after["Item.Key"]) or \
            not np.array_equal(_world_ids(start), _world_ids(after))


# ---- 10. growth ---------------------------------------------------------------------
def test_growth(built, monkeypatch):
    """The write is made before the tables grow."""
    monkeypatch.setenv("MADRONA_MWHIP_INITIAL_CAPACITY_DIV", "4")
    rt = runtime_lib()
    rt.mwhip_num_table_growths.restype = C.c_uint32
    rt.mwhip_num_table_growths.argtypes = [C.c_void_p]
    rng = np.random.default_rng(1000)
    columns = ["Item.Key", "Item.Vec3", "Item.Wide", "Item.Tag8"]
    with _sort_stress(worlds=300, flags=2) as s, \
            s.world_write("Item", columns, max_rows=40) as write:
        s.step(3)
        take = _random_take(rng, 300, 40)
        slabs = _fill(write, rng, take)
        _apply_and_check(s, write, slabs, take, "before the growth")
        grown = rt.mwhip_num_table_growths(s.hip_exec())
        rows_then = len(s.dump_column_raw(_index(s, "Item.Key"), RAW_CAP))
        s.step(37)
        assert rt.mwhip_num_table_growths(s.hip_exec()) > grown, "nothing grew"
        take = _random_take(rng, 300, 40)
        slabs = _fill(write, rng, take)
        _, after, counts = _apply_and_check(s, write, slabs, take, "after the growth")
        assert len(after["Item.Key"]) > rows_then and counts.sum() == len(after["Item.Key"])


# ---- 11. refusals -------------------------------------------------------------------
def _ids(sim, name):
    arch, comp = C.c_uint32(0), C.c_uint32(0)
    assert sim.lib.sim_hip_column_ids(sim.handle, _index(sim, name), C.byref(arch),
                                      C.byref(comp)) == 0
    return arch.value, comp.value


def test_refusals(built):
    """Each refusal with its message; every one of them returns before anything
    is allocated (the handle out is not touched) and changes nothing: the table,
    the launch list and a write that was there all along are what they were."""
    rt = runtime_lib()
    rng = np.random.default_rng(1100)
    with _sort_stress(worlds=3) as s, _sort_stress(worlds=3) as other:
        keeper = s.world_write("Item", max_rows=40)
        s.step(1)
        exec_ = s.hip_exec()
        item, key = _ids(s, "Item.Key")
        scratch, _ = _ids(s, "Scratch.Key")
        _, wide = _ids(s, "Item.Wide")
        _, tag8 = _ids(s, "Item.Tag8")
        assert _ids(s, "Item.Entity") == (item, 0) and _ids(s, "Item.WorldID") == (item, 1)
        launches = [k["name"] for k in s.profile(1)]
        s.step(1)
        table = _dump_table(s)

        def create(archetype, comps, max_rows, n=None):
            arr = (C.c_uint32 * max(len(comps), 1))(*comps)
            out = C.c_uint64(99)
            rc = rt.mwhip_write_create(exec_, archetype, arr, len(comps) if n is None else n,
                                       max_rows, C.byref(out))
            return rc, out.value, rt.mwhip_last_error().decode()

        for archetype, comps, max_rows, n, word in (
                (item, [key], 4, 0, "n == 0"),
                (item, [key] * 33, 4, None, "at most 32"),
                (item, [key], 0, None, "max_rows == 0"),
                (250, [key], 4, None, "archetype 250 is not registered"),
                (scratch, [wide], 4, None, "has no component %d" % wide),
                (item, [key, wide, key], 4, None, "component %d is listed twice" % key),
                (item, [key, 0], 4, None, "Entity column"),
                (item, [1, key], 4, None, "WorldID column")):
            rc, out, message = create(archetype, comps, max_rows, n)
            assert rc != 0 and out == 99 and word in message, (comps[:3], rc, out, message)
            assert message.startswith("write_create"), message
        # the wrapper hands the runtime's message on
        for name in ("Item.Entity", "Item.WorldID"):
            try:
                s.world_write("Item", ["Item.Key", name], max_rows=4)
            except RuntimeError as err:
                assert name.split(".")[1] + " column" in str(err), err
            else:
                raise AssertionError("a write of " + name)
        assert s._writes == [keeper]

        # handles: a column index out of range, another executor's, a destroyed one
        rc, handle, message = create(item, [key, wide, tag8], 4)
        assert rc == 0 and handle not in (0, 99), message
        assert rt.mwhip_write_apply(exec_, handle) == 0
        nbytes, cell = C.c_uint64(0), C.c_uint32(0)
        assert rt.mwhip_write_buffer(exec_, handle, 1, C.byref(nbytes), C.byref(cell))
        assert (nbytes.value, cell.value) == (3 * 4 * 240, 240)
        assert rt.mwhip_write_buffer(exec_, handle, 3, C.byref(nbytes), C.byref(cell)) is None
        assert "column 3 of 3" in rt.mwhip_last_error().decode()
        assert (nbytes.value, cell.value) == (3 * 4 * 240, 240)
        for call in (lambda: rt.mwhip_write_apply(other.hip_exec(), handle),
                     lambda: rt.mwhip_write_apply_async(other.hip_exec(), handle),
                     lambda: rt.mwhip_set_step_write(other.hip_exec(), handle, 1)):
            assert call() == -3
            assert "write %d is not one of this executor's" % handle in \
                rt.mwhip_last_error().decode()
        assert rt.mwhip_write_take(other.hip_exec(), handle) is None
        rt.mwhip_write_destroy(other.hip_exec(), handle)    # (not its: nothing happens)
        assert rt.mwhip_write_take(exec_, handle) and rt.mwhip_write_counts(exec_, handle)
        rt.mwhip_write_destroy(exec_, handle)
        for call in (lambda: rt.mwhip_write_apply(exec_, handle),
                     lambda: rt.mwhip_write_apply_async(exec_, handle),
                     lambda: rt.mwhip_set_step_write(exec_, handle, 1)):
            assert call() == -3
            assert "write %d is not one of this executor's" % handle in \
                rt.mwhip_last_error().decode()
        assert rt.mwhip_write_buffer(exec_, handle, 0, None, None) is None
        assert rt.mwhip_write_take(exec_, handle) is None
        assert rt.mwhip_write_counts(exec_, handle) is None

        # nothing changed: the table, the launches, and the write that was there
        _same_table(_dump_table(s), table, "after the refusals")
        assert [k["name"] for k in other.profile(1)] == launches
        assert [k["name"] for k in s.profile(1)] == launches
        take = np.array([40, 1, -1], np.int32)
        slabs = _fill(keeper, rng, take)
        _apply_and_check(s, keeper, slabs, take, "the keeper")
        s.step(2)
    # Simulator.close() orphaned it
    try:
        keeper.apply()
    except RuntimeError as err:
        assert "closed" in str(err)
    else:
        raise AssertionError("a world write outlived its simulator")
    keeper.close()
