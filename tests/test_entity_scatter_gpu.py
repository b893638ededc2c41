"""GPU: entity scatters (mwhip_scatter_*, Simulator.entity_scatter,
csrc/entity_scatter.hip) against madrona_amd/scatter_ref.py.  The core check
dumps every column the dump list can name of EVERY registered table of the
executor in table order (mwhip_dump_column_raw; Entity and WorldID of tables the
dump list does not show too), fills the buffers and select with seeded random
bytes, applies, dumps again and compares every byte of every column of every
table with scatter_ref over the first dump, and archetype, world and written."""
import ctypes as C
import os

import numpy as np
import pytest

from madrona_amd.gather_ref import read_handles, table_of_raw
from madrona_amd.scatter_ref import scatter_ref
from madrona_amd.simlib import (GatherSource, Simulator, hip_lib_path, ref_lib_path,
                                runtime_lib)

pytestmark = pytest.mark.gpu

CHURN_ONLY = 1      # sort_stress: churn without the compaction behind it
SORT_BY_KEY = 2     # sort_stress: a sort of Item by Key (no world-sorted prefix is left)
COMPACT_ONLY = 3    # sort_stress: the compaction that has to follow it
RAW_CAP = 1 << 16   # rows a table-order dump has room for
MAX_ARCHETYPES = 256
NONE = (0xFFFFFFFF, 0xFFFFFFFF)     # Entity::none()
# Item's components a scatter may list: cells of 1, 2, 4, 8, 12, 16, 20 and 240
# bytes, lane teams of 1, 2 and 16
ITEM = ["Tag8", "Half", "Key", "Pair", "Vec3", "Quad", "Blob20", "Wide"]


def _need_ref(sim):
    if not os.path.exists(ref_lib_path(sim)):
        pytest.skip("oracle/_ref missing on this box")


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _rt():
    rt = runtime_lib()
    rt.mwhip_num_rows.restype = C.c_int32
    rt.mwhip_num_rows.argtypes = [C.c_void_p, C.c_uint32]
    rt.mwhip_dump_column_raw.restype = C.c_int64
    rt.mwhip_dump_column_raw.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                         C.c_uint64]
    rt.mwhip_num_table_growths.restype = C.c_uint32
    rt.mwhip_num_table_growths.argtypes = [C.c_void_p]
    return rt


def _sort_stress(worlds=33, seed=7, flags=0):
    return Simulator(hip_lib_path("sort_stress"), worlds, seed=seed, flags=flags)


def _ids(sim, name):
    """(archetype id, component id) of dump-list column `name`"""
    arch, comp = C.c_uint32(0), C.c_uint32(0)
    idx = [c[0] for c in sim.columns].index(name)
    assert sim.lib.sim_hip_column_ids(sim.handle, idx, C.byref(arch), C.byref(comp)) == 0
    return arch.value, comp.value


def _all_components(sim):
    """{name: (component id, cell bytes)} of every component the dump list
    names, Entity and WorldID left out (every table has them)"""
    out = {}
    for column in sim.columns:
        name = column[0].split(".", 1)[1]
        if name in ("Entity", "WorldID") or name in out:
            continue
        out[name] = (_ids(sim, column[0])[1], column[1])
    return out


def _raw(sim, archetype, component, cell):
    """Column `component` of table `archetype` in table order, or None if the
    table has no such column."""
    rt = _rt()
    buf = np.empty(RAW_CAP * cell, dtype=np.uint8)
    n = rt.mwhip_dump_column_raw(sim.hip_exec(), archetype, component, buf.ctypes.data, buf.nbytes)
    if n == -1 and "has no component" in rt.mwhip_last_error().decode():
        return None
    assert n >= 0, (archetype, component, n, rt.mwhip_last_error().decode())
    return buf[: n * cell].reshape(n, cell).copy()


def _tables(sim):
    """Every registered table of the executor with its Entity and WorldID
    columns and every other column the dump list can name, in table order."""
    rt = _rt()
    comps = _all_components(sim)
    tables = []
    for a in range(MAX_ARCHETYPES):
        if rt.mwhip_num_rows(sim.hip_exec(), a) < 0:
            continue
        columns = {}
        for name, (comp, cell) in comps.items():
            cells = _raw(sim, a, comp, cell)
            if cells is not None:
                columns[name] = cells
        tables.append(table_of_raw(a, _raw(sim, a, 0, 8), _raw(sim, a, 1, 4), columns))
    return tables


def _same_tables(got, want, what):
    assert [t.archetype for t in got] == [t.archetype for t in want], what
    for g, w in zip(got, want):
        assert np.array_equal(g.entities, w.entities), (what, g.archetype, "Entity")
        assert np.array_equal(g.world_ids, w.world_ids), (what, g.archetype, "WorldID")
        assert list(g.columns) == list(w.columns), (what, g.archetype)
        for name in w.columns:
            assert g.columns[name].shape == w.columns[name].shape, (what, g.archetype, name)
            bad = np.argwhere(g.columns[name] != w.columns[name])
            assert len(bad) == 0, (what, "table", g.archetype, name, len(bad),
                                   "bytes differ, first (row, byte):", bad[:4].tolist())


def _fill(scatter, rng, select=None):
    """seeded random bytes into every buffer and (unless given) select; what
    was put there"""
    torch = _torch()
    n = scatter.num_handles
    inputs = {}
    for name in scatter.components:
        inputs[name] = rng.integers(0, 256, (n, scatter.cell_bytes(name))).astype(np.uint8)
        scatter.tensor(name).copy_(torch.from_numpy(inputs[name]).cuda())
    if select is None:
        # (any non-zero word selects)
        select = rng.integers(0, 2, n) * rng.integers(-5, 6, n)
        select[rng.integers(0, n, max(n // 8, 1))] = 0x40000000
    select = np.asarray(select, dtype=np.int32)
    assert select.shape == (n,)
    scatter.select.copy_(torch.from_numpy(select).cuda())
    torch.cuda.synchronize()
    return inputs, select


def _apply_and_check(sim, scatter, handles, rng, what, select=None, before=None):
    """The core check.  Returns (archetype, world, written, select, the tables before,
    the tables after)."""
    assert len(handles) == scatter.num_handles
    if before is None:
        before = _tables(sim)
    inputs, select = _fill(scatter, rng, select)
    # the outputs are rewritten in full by every apply
    for out in (scatter.archetypes, scatter.worlds, scatter.written):
        out.fill_(77)
    _torch().cuda.synchronize()
    assert scatter.apply() is scatter
    after = _tables(sim)
    archetype, world, written, want = scatter_ref(handles, select, before, inputs)
    for got, ref, label in ((scatter.archetypes, archetype, "archetype"),
                            (scatter.worlds, world, "world"),
                            (scatter.written, written, "written")):
        got = got.cpu().numpy()
        assert got.dtype == np.int32 and got.shape == ref.shape, (what, label)
        bad = np.flatnonzero(got != ref)
        assert len(bad) == 0, (what, label, "differs at handles", bad[:4].tolist(),
                               got[bad[:4]].tolist(), ref[bad[:4]].tolist())
    _same_tables(after, want, what)
    # the inputs are the caller's
    for name in scatter.components:
        assert np.array_equal(scatter.tensor(name).cpu().numpy(), inputs[name]), (what, name)
    assert np.array_equal(scatter.select.cpu().numpy(), select), what
    return archetype, world, written, select, before, after


def _slab_handles(view, name, first_byte=0, handles=1):
    """the handles a scatter over view.handle_source(...) reads, from the slab"""
    view.compute()
    ptr, records, record_bytes, first, per = view.handle_source(name, first_byte, handles)
    return read_handles(view.tensor(name).cpu().numpy(), records, record_bytes, first, per)


def _device_handles(handles):
    """uint32 [N, 2] as a torch int32 [N, 2] on the device"""
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(handles).view(np.int32).copy()).cuda()


def _live_entities(tables, archetype=None):
    """uint32 [n, 2]: the handles of the live rows that hold an entity"""
    out = []
    for t in tables:
        if archetype is not None and t.archetype != archetype:
            continue
        keep = (t.world_ids != -1) & (t.entities[:, 1] < 2 ** 31)
        out.append(t.entities[keep])
    return np.concatenate(out)


# ---- 1. widths, teams, a partial last wave ------------------------------------------
def test_every_cell_width_and_team_size(built):
    rng = np.random.default_rng(100)
    with _sort_stress() as s, s.world_view("Item", ["Item.Entity"], max_rows=40) as hv, \
            s.entity_scatter(hv.handle_source("Item.Entity"), ITEM) as sc:
        assert sc.num_handles == 33 * 40 == 1320 and sc.num_handles % 64 != 0
        assert [sc.cell_bytes(n) for n in ITEM] == [1, 2, 4, 8, 12, 16, 20, 240]
        # all zero at creation: an apply before anything is filled writes nothing
        s.step(3)
        handles = _slab_handles(hv, "Item.Entity")
        before = _tables(s)
        sc.apply()
        _same_tables(_tables(s), before, "an apply of a fresh scatter")
        assert not sc.written.cpu().numpy().any()
        archetype, world, written, select, before, after = _apply_and_check(
            s, sc, handles, rng, "step 3", before=before)
        item = _ids(s, "Item.Key")[0]
        assert (archetype == item).sum() > 500 and 100 < written.sum() < (archetype >= 0).sum()
        changed = [name for name in ITEM
                   if not np.array_equal(next(t for t in after if t.archetype == item).columns[name],
                                         next(t for t in before if t.archetype == item).columns[name])]
        assert changed == ITEM
        # typed tensors over the same bytes
        vec3 = sc.tensor("Vec3", np.float32)
        assert tuple(vec3.shape) == (1320, 3)
        assert np.array_equal(vec3.cpu().numpy().view(np.uint8).reshape(1320, 12),
                              sc.tensor("Vec3").cpu().numpy())


def test_the_pinned_exported_column(built):
    """flags bit 6: Item.Vec3 is an exported column, which the sort keeps in
    place; the exported tensor shows the scattered bytes."""
    rng = np.random.default_rng(110)
    with _sort_stress(flags=64) as s, s.world_view("Item", ["Item.Entity"], max_rows=40) as hv, \
            s.entity_scatter(hv.handle_source("Item.Entity"), ["Vec3", "Tag8"]) as sc:
        s.step(2)
        pin_ptr = s.tensor_ptr("item_vec3")
        handles = _slab_handles(hv, "Item.Entity")
        archetype, _, written, _, before, after = _apply_and_check(s, sc, handles, rng, "pinned")
        item = next(t for t in after if t.archetype == _ids(s, "Item.Vec3")[0])
        n = len(item.world_ids)
        assert s.tensor_ptr("item_vec3") == pin_ptr and written.sum() > 100
        exported = s.read_tensor("item_vec3")[:n]
        assert np.array_equal(exported.view(np.uint8).reshape(n, 12), item.columns["Vec3"])


# ---- 2. edges of N, duplicates, collisions -----------------------------------------
def test_edges_of_n_and_claim_table_collisions(built):
    """N = 1, 63, 64, 65, 130 and 33 distinct entities, all selected: every one
    of them is written.  33 and 65 keys in 128 and 256 slots... any N keys in
    the power of two >= 2N slots collide under any hash function sooner or
    later; 65 and 130 of them over two and three wavefronts."""
    rng = np.random.default_rng(200)
    with _sort_stress() as s:
        s.step(3)
        tables = _tables(s)
        pool = _live_entities(tables, _ids(s, "Item.Key")[0])
        assert len(pool) >= 130 and len({tuple(h) for h in pool.tolist()}) == len(pool)
        for n in (1, 33, 63, 64, 65, 130):
            handles = pool[rng.permutation(len(pool))[:n]]
            kept = _device_handles(handles)
            with s.entity_scatter(kept, ["Key", "Wide", "Blob20"]) as sc:
                assert sc.num_handles == n
                _, _, written, _, _, _ = _apply_and_check(
                    s, sc, handles, rng, ("distinct", n), select=np.ones(n, np.int32))
                assert written.tolist() == [1] * n
                _apply_and_check(s, sc, handles, rng, ("distinct, random select", n))


def test_duplicates(built):
    rng = np.random.default_rng(300)
    with _sort_stress() as s:
        s.step(3)
        pool = _live_entities(_tables(s), _ids(s, "Item.Key")[0])
        base = pool[:130].copy()
        ones = np.ones(130, np.int32)

        def run(handles, select, what):
            kept = _device_handles(handles)
            with s.entity_scatter(kept, ["Key", "Vec3", "Wide"]) as sc:
                return _apply_and_check(s, sc, handles, rng, what, select=select)[2]

        # inside one wavefront
        handles = base.copy()
        handles[40] = handles[3]
        handles[41] = handles[3]
        written = run(handles, ones, "inside a wavefront")
        assert written[[3, 40, 41]].tolist() == [0, 0, 1] and written.sum() == 128
        # across wavefronts: handle 0 and handle 129 the same entity
        handles = base.copy()
        handles[129] = handles[0]
        written = run(handles, ones, "across wavefronts")
        assert written[0] == 0 and written[129] == 1 and written.sum() == 129
        # every handle the same entity
        handles = np.repeat(base[7:8], 130, axis=0)
        written = run(handles, ones, "all the same")
        assert written.tolist() == [0] * 129 + [1]
        select = ones.copy()
        select[100:] = 0
        written = run(handles, select, "all the same, the last 30 unselected")
        assert written.tolist() == [0] * 99 + [1] + [0] * 30
        # a duplicate whose later copy is unselected
        handles = base.copy()
        handles[129] = handles[0]
        handles[50] = handles[20]
        select = ones.copy()
        select[129] = 0
        select[50] = 0
        written = run(handles, select, "the later copy unselected")
        assert written[[0, 129, 20, 50]].tolist() == [1, 0, 1, 0]
        # many duplicates, random select
        handles = base[rng.integers(0, 20, 130)]
        run(handles, None, "130 handles of 20 entities")


# ---- 3. handles that name nothing ---------------------------------------------------
def test_handles_that_name_nothing_change_no_byte(built):
    """Entity::none(), handles kept across churn steps that went stale, ids at and
    past entityCapacity, a free slot's {0, id}, a live id with another
    generation: all selected, no byte of any table changes.  The zero padding
    of a view's slab is the handle {0, 0}: in sort_stress a live entity holds
    it, so the padding is 70 copies of one handle that names that entity."""
    with _sort_stress() as s, s.world_view("Item", ["Item.Entity"], max_rows=40) as hv:
        s.step(2)
        old = _slab_handles(hv, "Item.Entity")
        counts = hv.counts.cpu().numpy()
        padding = np.tile(np.arange(40), 33) >= np.repeat(counts, 40)
        assert padding.sum() > 64 and not old[padding].any()
        s.step(5)           # (churn)
        tables = _tables(s)
        live = {tuple(h) for h in _live_entities(tables).tolist()}
        gens = {ident: gen for gen, ident in live}
        stale = np.array([h for h in old[~padding].tolist() if tuple(h) not in live], np.uint32)
        assert len(stale) >= 32, "no handle of step 2 went stale"
        past = (max(gens) // 64 + 1) * 64
        free = np.array([(0, ident) for ident in range(max(gens)) if ident not in gens][:16],
                        np.uint32).reshape(-1, 2)
        assert len(free) >= 1, "no free id below the highest one in use"
        live_gen, live_id = next(iter(live))
        extras = np.array([NONE, (0, 2 ** 31 - 1), (0, 0xFFFFFFFE), (0, past), (7, past + 640),
                           (0, 1 << 30), ((live_gen + 1) & 0xFFFFFFFF, live_id)], np.uint32)
        rng = np.random.default_rng(400)
        handles = np.concatenate([stale, free, extras])
        kept = _device_handles(handles)
        with s.entity_scatter(kept, ITEM) as sc:
            archetype, world, written, _, before, after = _apply_and_check(
                s, sc, handles, rng, "handles that name nothing",
                select=np.ones(len(handles), np.int32), before=tables)
            assert (archetype == -1).all() and (world == -1).all() and not written.any()
            _same_tables(after, before, "no byte anywhere")

        # the zero padding of the slab, between the handles above
        handles = np.concatenate([stale[:20], old[padding][:70], extras])
        kept = _device_handles(handles)
        with s.entity_scatter(kept, ITEM) as sc:
            archetype, world, written, _, before, after = _apply_and_check(
                s, sc, handles, rng, "zero padding",
                select=np.ones(len(handles), np.int32), before=tables)
            assert (archetype[:20] == -1).all() and (archetype[90:] == -1).all()
            if (0, 0) in live:
                # one entity, 70 times: the last copy wins and one row changes
                assert (archetype[20:90] >= 0).all() and len(set(archetype[20:90])) == 1
                assert written.tolist() == [0] * 89 + [1] + [0] * len(extras)
                # (of the table that entity is in, which need not have a listed column)
                rows = {(a.archetype, int(r)) for a, b in zip(after, before) for n in a.columns
                        for r in np.flatnonzero((a.columns[n] != b.columns[n]).any(axis=1))}
                home = next(t for t in before if t.archetype == archetype[20])
                assert len(rows) == (1 if set(ITEM) & set(home.columns) else 0), rows
                assert all(a == archetype[20] for a, _ in rows)
            else:
                assert (archetype == -1).all() and not written.any()
                _same_tables(after, before, "no byte anywhere")


# ---- 4. two kinds of entity, a component one of them lacks --------------------------
def test_tables_without_a_listed_column(built):
    """Handles of Item and of Reuse0 .. Reuse4 (flags 128; Key and Pair, no Wide)
    in one list, Key and Wide listed: a Reuse entity gets its Key and counts as
    written.  Scratch's rows are temporaries, whose cells name nothing."""
    rng = np.random.default_rng(500)
    with _sort_stress(flags=128) as s:
        s.step(3)
        item, scratch = _ids(s, "Item.Key")[0], _ids(s, "Scratch.Key")[0]
        reuse = [_ids(s, "Reuse%d.Key" % k)[0] for k in range(5)]
        tables = {t.archetype: t for t in _tables(s)}
        for a in reuse:
            assert "Wide" not in tables[a].columns and "Key" in tables[a].columns
        item_handles = tables[item].entities[:100]
        scratch_handles = tables[scratch].entities[:30]
        reuse_handles = np.concatenate([tables[a].entities for a in reuse])
        assert len(reuse_handles) > 64
        assert (scratch_handles == np.array(NONE, dtype=np.uint32)).all()
        handles = np.concatenate([item_handles, scratch_handles, reuse_handles, reuse_handles[:9]])
        handles = handles[rng.permutation(len(handles))]
        kept = _device_handles(handles)
        with s.entity_scatter(kept, ["Key", "Wide"]) as sc:
            archetype, _, written, select, before, after = _apply_and_check(
                s, sc, handles, rng, "Item + Scratch + Reuse")
            in_reuse = np.isin(archetype, reuse)
            assert in_reuse.sum() == len(reuse_handles) + 9 and written[in_reuse].sum() > 5
            assert (archetype == item).sum() == 100 and (archetype == -1).sum() == 30
            before = {t.archetype: t for t in before}
            for t in after:
                if t.archetype in reuse and len(t.world_ids):
                    assert np.array_equal(t.columns["Pair"], before[t.archetype].columns["Pair"])
        # only Wide listed: nothing of a Reuse table changes, written is 1 all the same
        handles = reuse_handles
        kept = _device_handles(handles)
        with s.entity_scatter(kept, ["Wide"]) as sc:
            _, _, written, _, before, after = _apply_and_check(
                s, sc, handles, rng, "Reuse, Wide alone", select=np.ones(len(handles), np.int32))
            assert written.tolist() == [1] * len(handles)
            _same_tables(after, before, "Reuse, Wide alone")


# ---- 5. handles inside wider cells --------------------------------------------------
def test_four_handles_per_door_properties_cell(built):
    rng = np.random.default_rng(600)
    with Simulator(hip_lib_path("escape_room"), 5, seed=5) as s, \
            s.world_view("DoorEntity", ["DoorEntity.DoorProperties"], max_rows=4) as dv:
        s.step(3)
        assert dv.cell_bytes("DoorEntity.DoorProperties") == 40
        source = dv.handle_source("DoorEntity.DoorProperties", first_byte=0, handles=4)
        assert source[1:] == (5 * 4, 40, 0, 4)
        with s.entity_scatter(source, ["Position", "ButtonState"]) as sc:
            assert sc.num_handles == 80
            handles = _slab_handles(dv, "DoorEntity.DoorProperties", 0, 4)
            archetype, world, written, _, before, after = _apply_and_check(
                s, sc, handles, rng, "the doors' buttons",
                select=np.ones(80, np.int32))
            button = _ids(s, "ButtonEntity.ButtonState")[0]
            assert (archetype == button).sum() >= 15
            assert written.sum() >= 5 and (written <= (archetype >= 0)).all()
            _apply_and_check(s, sc, handles, rng, "the doors' buttons, random select")

        # records of 24 bytes with one handle at byte 8, the rest never read as one
        torch = _torch()
        pool = _live_entities(_tables(s))
        chosen = pool[rng.integers(0, len(pool), 150)]
        chosen[::7] = NONE
        records = np.full((150, 24), 0xCD, dtype=np.uint8)
        records[:, 8:16] = chosen.view(np.uint8).reshape(150, 8)
        buf = torch.from_numpy(records).cuda()
        with s.entity_scatter((buf.data_ptr(), 150, 24, 8, 1), ["Position", "Rotation"]) as sc:
            archetype, _, _, _, _, _ = _apply_and_check(s, sc, chosen, rng, "24-byte records")
            assert len(np.unique(archetype)) >= 4       # nothing, and three kinds of entity
        assert np.array_equal(buf.cpu().numpy(), records)


# ---- 6. tables that are not sorted --------------------------------------------------
def test_holes_a_tail_no_prefix_and_the_twin_swap(built):
    """One scatter over three graphs: churn without compaction (a sorted prefix
    with holes, rows behind it), a sort by key (no prefix; the columns swap with
    their twins) and the compaction after it (they swap again)."""
    rng = np.random.default_rng(700)
    names = ["Pair", "Vec3", "Wide", "Tag8"]
    with _sort_stress() as s, s.world_view("Item", ["Item.Entity"], max_rows=40) as hv:
        s.step(4)
        old_handles = _slab_handles(hv, "Item.Entity")
        kept = _device_handles(old_handles)
        item_id = _ids(s, "Item.Key")[0]
        with s.entity_scatter(hv.handle_source("Item.Entity"), names) as fresh, \
                s.entity_scatter(kept, names) as old:
            saw_destroyed = saw_tail = False
            for what, graph in (("churn 0", CHURN_ONLY), ("churn 1", CHURN_ONLY),
                                ("sorted by key", SORT_BY_KEY), ("compacted", COMPACT_ONLY)):
                s.run_taskgraph(graph)
                _apply_and_check(s, fresh, _slab_handles(hv, "Item.Entity"), rng, ("fresh", what))
                archetype, _, written, _, _, after = _apply_and_check(
                    s, old, old_handles, rng, ("old", what))
                item = next(t for t in after if t.archetype == item_id)
                if what.startswith("churn"):
                    assert (item.world_ids == -1).any(), "no destroyed row in the raw table"
                    saw_tail |= bool((np.diff(item.world_ids) < 0).any())
                    live = {tuple(h) for h in _live_entities([item]).tolist()}
                    gone = [i for i, h in enumerate(old_handles.tolist())
                            if tuple(h) != (0, 0) and tuple(h) not in live]
                    saw_destroyed |= bool(gone)
                    assert (archetype[gone] == -1).all() and not written[gone].any()
                if what == "sorted by key":
                    live = item.world_ids[item.world_ids >= 0]
                    assert (np.diff(live) < 0).sum() > len(live) // 4, "the worlds stayed grouped"
            assert saw_destroyed, "no handle of step 4 named a row that was destroyed in place"
            assert saw_tail, "no row behind the sorted prefix"
            s.step(1)
            _apply_and_check(s, fresh, _slab_handles(hv, "Item.Entity"), rng, "the next full step")


# ---- 7. growth after create ---------------------------------------------------------
def test_ids_taken_at_run_time_after_create(built):
    """Cold start: some worlds take their first block of entity ids at run time,
    behind every id handed out at init."""
    rng = np.random.default_rng(800)
    with _sort_stress(flags=1) as s, s.world_view("Item", ["Item.Entity"], max_rows=40) as hv, \
            s.entity_scatter(hv.handle_source("Item.Entity"), ["Key", "Wide"]) as sc:
        ids = _live_entities(_tables(s))[:, 1]
        init_end = (int(ids.max()) // 64 + 1) * 64 if len(ids) else 0
        s.step(10)
        handles = _slab_handles(hv, "Item.Entity")
        archetype, _, written, _, _, _ = _apply_and_check(s, sc, handles, rng, "cold start")
        late = (handles[:, 1].astype(np.int64) >= init_end) & (written == 1)
        assert late.any(), ("no id behind the ids of init was written", init_end)


def test_tables_that_grew_after_create(built, monkeypatch):
    """Ramp-up: the tables grow at run time."""
    monkeypatch.setenv("MADRONA_MWHIP_INITIAL_CAPACITY_DIV", "4")
    rt = _rt()
    rng = np.random.default_rng(810)
    with _sort_stress(worlds=300, flags=2) as s, \
            s.world_view("Item", ["Item.Entity"], max_rows=40) as hv, \
            s.entity_scatter(hv.handle_source("Item.Entity"), ["Key", "Vec3", "Wide", "Tag8"]) as sc:
        grown = rt.mwhip_num_table_growths(s.hip_exec())
        rows = rt.mwhip_num_rows(s.hip_exec(), _ids(s, "Item.Key")[0])
        _apply_and_check(s, sc, _slab_handles(hv, "Item.Entity"), rng, "before the growth")
        s.step(40)
        assert rt.mwhip_num_table_growths(s.hip_exec()) > grown, "nothing grew"
        assert rt.mwhip_num_rows(s.hip_exec(), _ids(s, "Item.Key")[0]) > 4 * rows
        archetype, _, written, _, _, _ = _apply_and_check(
            s, sc, _slab_handles(hv, "Item.Entity"), rng, "after the growth")
        assert (archetype >= 0).sum() > 4 * rows and written.sum() > rows


# ---- 8. round trip ------------------------------------------------------------------
def test_a_gather_scattered_back_changes_nothing(built):
    torch = _torch()
    names = ["Tag8", "Key", "Vec3", "Blob20", "Wide"]
    with _sort_stress() as s, s.world_view("Item", ["Item.Entity"], max_rows=40) as hv, \
            s.entity_gather(hv.handle_source("Item.Entity"), names) as g, \
            s.entity_scatter(hv.handle_source("Item.Entity"), names) as sc, \
            s.digest() as digest:
        s.step(3)
        hv.compute()
        before = _tables(s)
        digest_before = digest.compute().copy()
        g.compute()
        for name in names:
            assert sc.tensor(name).shape == g.tensor(name).shape
            sc.tensor(name).copy_(g.tensor(name))
        sc.select.fill_(1)
        torch.cuda.synchronize()
        sc.apply()
        _same_tables(_tables(s), before, "a gather scattered back")
        assert np.array_equal(digest.compute(), digest_before)
        assert np.array_equal(sc.archetypes.cpu().numpy(), g.archetypes.cpu().numpy())
        assert np.array_equal(sc.worlds.cpu().numpy(), g.worlds.cpu().numpy())
        assert sc.written.cpu().numpy().sum() > 500


# ---- 9. against the reference backend -----------------------------------------------
def test_scattering_the_references_values_keeps_lock_step(built):
    """Three steps in lock step, Position and Rotation of every agent of the HIP
    side overwritten with 0x3C bytes through the reference's own handles, then
    with the reference's own values, five more steps in lock step, bit for bit."""
    _need_ref("escape_room")
    torch = _torch()
    W = 5
    rng = np.random.default_rng(900)
    with Simulator(ref_lib_path("escape_room"), W, seed=5, num_workers=1) as ref, \
            Simulator(hip_lib_path("escape_room"), W, seed=5) as hip:
        ref_names = [c[0] for c in ref.columns]
        hip_names = [c[0] for c in hip.columns]
        columns = [n for n in hip_names if n in ref_names]
        assert "Agent.Position" in columns and "Agent.Rotation" in columns

        def act():
            a = np.stack([rng.integers(0, 4, (W, 2)), rng.integers(0, 8, (W, 2)),
                          rng.integers(-2, 3, (W, 2)), np.zeros((W, 2), int)],
                         -1).astype(np.int32)
            ref.write_tensor("action", a)
            hip.write_tensor("action", a)
            ref.step(1)
            hip.step(1)

        def lock_step(what):
            for col in columns:
                ref_rows, ref_counts = ref.dump_column(ref_names.index(col), 512)
                hip_rows, hip_counts = hip.dump_column(hip_names.index(col), 512)
                assert np.array_equal(ref_counts, hip_counts), (what, col)
                assert np.array_equal(ref_rows, hip_rows), (what, col)

        for _ in range(3):
            act()
        lock_step("before")
        dump = ref.dump_all(512)
        handles = read_handles(dump["Agent.Entity"][0], 2 * W, 8)
        kept = _device_handles(handles)
        with hip.entity_scatter(kept, ["Position", "Rotation"]) as sc:
            sc.tensor("Position").fill_(0x3C)
            sc.tensor("Rotation").fill_(0x3C)
            sc.select.fill_(1)
            torch.cuda.synchronize()
            sc.apply()
            assert sc.written.cpu().numpy().tolist() == [1] * (2 * W)
            assert sc.archetypes.cpu().numpy().tolist() == [_ids(hip, "Agent.Position")[0]] * (2 * W)
            spoiled, _ = hip.dump_column(hip_names.index("Agent.Position"), 512)
            assert (spoiled == 0x3C).all() and len(spoiled) == 2 * W
            for name in ("Position", "Rotation"):
                rows, counts = dump["Agent." + name]
                assert counts.tolist() == [2] * W
                sc.tensor(name).copy_(torch.from_numpy(np.ascontiguousarray(rows)).cuda())
            torch.cuda.synchronize()
            sc.apply()
        lock_step("scattered back")
        for step in range(5):
            act()
            lock_step(("step", step))


# ---- 10. step scatters --------------------------------------------------------------
def _slots(n):
    slots = 2
    while slots < 2 * n:
        slots *= 2
    return slots


def test_the_step_scatter_launches(built):
    """Three launches, behind the input rings and the step writes and in front
    of the first node; none when no step scatter is set."""
    torch = _torch()
    rt = runtime_lib()
    rng = np.random.default_rng(1000)
    with _sort_stress() as s, s.world_write("Item", ["Item.Pair"], max_rows=40) as write:
        s.step(2)
        pool = _live_entities(_tables(s), _ids(s, "Item.Key")[0])
        handles = pool[rng.integers(0, 100, 130)]
        kept = _device_handles(handles)
        names = lambda: [k["name"] for k in s.profile(1)]   # noqa: E731
        before = names()
        assert not [n for n in before if n.startswith("scatter:")]
        three = ["scatter:scatter.zero", "scatter:scatter.claim", "scatter:scatter.write"]
        with s.entity_scatter(kept, ["Key", "Wide"]) as sc:
            # made, not set: every launch list is what it was
            assert names() == before
            _fill(sc, rng)
            sc.every_step()
            stats = s.profile(1)
            during = [k["name"] for k in stats]
            assert during[:3] == three and during[3:] == before, during
            # algo_bytes: the claim table; per handle 20 bytes + 24 per named one; per
            # handle 16 + 24 per named one + per winner the listed cells twice
            n = 130
            named = int((sc.archetypes.cpu().numpy() >= 0).sum())
            won = int(sc.written.cpu().numpy().sum())
            assert 0 < won < named <= n
            assert stats[0]["algo_bytes"] == _slots(n) * 8 == 4096
            assert stats[1]["algo_bytes"] == n * 20 + named * 24, stats[1]
            assert stats[2]["algo_bytes"] == n * 16 + named * 24 + won * 2 * (4 + 240), stats[2]

            write.every_step()
            ring = torch.zeros((2, 130), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert rt.mwhip_set_input_ring(s.hip_exec(), sc.select_ptr, ring.data_ptr(),
                                           130 * 4, 2) == 0
            during = names()
            assert during[:5] == ["input:ring", "write:write"] + three, during
            assert during[5:] == before
            assert rt.mwhip_set_input_ring(s.hip_exec(), sc.select_ptr, None, 0, 0) == 0
            write.every_step(False)
            sc.every_step(False)
            assert names() == before
            sc.every_step()
        # destroying a set scatter unsets it
        assert names() == before
        s.step(1)


def test_input_rings_feed_the_step_scatter(built):
    """K queued steps carry K different injections: two 4-slot input rings feed
    select and the Key buffer of a step scatter whose handles have duplicates;
    a twin applies the four by hand between four single steps."""
    torch = _torch()
    rng = np.random.default_rng(1100)
    K, N = 4, 130
    rt = runtime_lib()
    with _sort_stress() as s, _sort_stress() as twin:
        s.step(2)
        twin.step(2)
        pool = _live_entities(_tables(s), _ids(s, "Item.Key")[0])
        handles = pool[rng.integers(0, 90, N)]
        kept, twin_kept = _device_handles(handles), _device_handles(handles)
        with s.entity_scatter(kept, ["Key"]) as sc, twin.entity_scatter(twin_kept, ["Key"]) as tsc:
            selects = rng.integers(0, 2, (K, N)).astype(np.int32)
            cells = rng.integers(0, 256, (K, N, 4)).astype(np.uint8)
            select_ring = torch.from_numpy(selects).cuda()
            cell_ring = torch.from_numpy(cells).cuda()
            torch.cuda.synchronize()
            sc.every_step()
            assert rt.mwhip_set_input_ring(s.hip_exec(), sc.select_ptr, select_ring.data_ptr(),
                                           N * 4, K) == 0
            assert rt.mwhip_set_input_ring(s.hip_exec(), sc.buffer_ptr("Key"),
                                           cell_ring.data_ptr(), N * 4, K) == 0
            s.step_async(K)
            outputs = []
            for k in range(K):
                tsc.select.copy_(torch.from_numpy(selects[k]).cuda())
                tsc.tensor("Key").copy_(torch.from_numpy(cells[k]).cuda())
                torch.cuda.synchronize()
                tsc.apply()
                outputs.append((tsc.archetypes.cpu().numpy(), tsc.written.cpu().numpy()))
                twin.step(1)
            s.sync()
            _same_tables(_tables(s), _tables(twin), "after the K steps")
            # the outputs are those of the last replay, the inputs its slot
            assert np.array_equal(sc.archetypes.cpu().numpy(), outputs[K - 1][0])
            assert np.array_equal(sc.written.cpu().numpy(), outputs[K - 1][1])
            assert np.array_equal(sc.select.cpu().numpy(), selects[K - 1])
            assert np.array_equal(sc.tensor("Key").cpu().numpy(), cells[K - 1])
            assert sum(int(o[1].sum()) for o in outputs) > K
            assert not np.array_equal(outputs[0][0], outputs[K - 1][0]), "nobody went stale"
            assert rt.mwhip_set_input_ring(s.hip_exec(), sc.select_ptr, None, 0, 0) == 0
            assert rt.mwhip_set_input_ring(s.hip_exec(), sc.buffer_ptr("Key"), None, 0, 0) == 0


def test_a_ninth_step_scatter_a_component_clash_and_destroying_a_set_one(built):
    torch = _torch()
    with _sort_stress(worlds=3) as s:
        s.step(1)
        buf = torch.zeros((16, 2), dtype=torch.int32, device="cuda")
        before = [k["name"] for k in s.profile(1)]
        single = ["Tag8", "Half", "Key", "Pair", "Vec3", "Quad", "Blob20", "Wide"]
        scatters = [s.entity_scatter(buf, [name]) for name in single]
        for sc in scatters:
            sc.every_step()
        launches = [k["name"] for k in s.profile(1)]
        assert [n for n in launches if n.startswith("scatter:")] == [
            "scatter:scatter.zero", "scatter:scatter.claim", "scatter:scatter.write"], launches
        # eight are set: a ninth is refused for being the ninth
        key_id = _ids(s, "Item.Key")[1]
        ninth = s.entity_scatter(buf, ["Key", "Wide"])
        with pytest.raises(RuntimeError) as err:
            ninth.every_step()
        assert "-> -2" in str(err.value) and "at most 8" in str(err.value)
        # seven are set: the clash is named
        scatters[7].close()        # (Wide; destroying a set scatter unsets it)
        with pytest.raises(RuntimeError) as err:
            ninth.every_step()
        assert "-> -2" in str(err.value), str(err.value)
        assert "lists component %d" % key_id in str(err.value), str(err.value)
        assert "step scatter %d lists already" % scatters[2].handle in str(err.value)
        assert [k["name"] for k in s.profile(1)] == launches
        scatters[2].every_step(False)
        ninth.every_step()
        scatters[2].every_step(False)      # (off already: nothing to do)
        with pytest.raises(RuntimeError) as err:
            scatters[2].every_step()
        assert "lists component %d" % key_id in str(err.value)
        s.step(2)       # (the step graph replays without the one destroyed)
        for sc in scatters[:7] + [ninth]:
            sc.close()
        assert [k["name"] for k in s.profile(1)] == before
        assert s._scatters == []
        s.step(1)


def test_apply_async_is_stream_ordered(built):
    rng = np.random.default_rng(1200)
    with _sort_stress() as s, _sort_stress() as twin:
        s.step(2)
        twin.step(2)
        start = _tables(s)
        handles = _live_entities(start, _ids(s, "Item.Key")[0])[:130]
        kept, twin_kept = _device_handles(handles), _device_handles(handles)
        with s.entity_scatter(kept, ["Key", "Wide"]) as sc, \
                twin.entity_scatter(twin_kept, ["Key", "Wide"]) as tsc:
            _fill(sc, np.random.default_rng(1201))
            s.step_async(3)
            sc.apply_async()
            s.sync()
            twin.step(3)
            archetype, _, written, _, _, after = _apply_and_check(
                twin, tsc, handles, np.random.default_rng(1201), "twin")
            _same_tables(_tables(s), after, "step_async(3), apply_async(), sync()")
            assert np.array_equal(sc.written.cpu().numpy(), written)
            assert np.array_equal(sc.archetypes.cpu().numpy(), archetype)
            # (applied to the tables of three steps later, not to those it was queued at)
            assert (archetype == -1).any() and written.any()


# ---- 11. refusals -------------------------------------------------------------------
def test_refusals(built):
    torch = _torch()
    rt = runtime_lib()
    with _sort_stress(worlds=3) as s, _sort_stress(worlds=3) as other:
        s.step(1)
        exec_ = s.hip_exec()
        key, wide = _ids(s, "Item.Key")[1], _ids(s, "Item.Wide")[1]
        buf = torch.zeros((16, 2), dtype=torch.int32, device="cuda")
        ptr = buf.data_ptr()

        def create(src, records, record_bytes, first, per, comps, n=None):
            source = GatherSource(src, records, record_bytes, first, per, 0)
            arr = (C.c_uint32 * max(len(comps), 1))(*comps)
            out = C.c_uint64(99)
            rc = rt.mwhip_scatter_create(exec_, C.byref(source), arr,
                                         len(comps) if n is None else n, C.byref(out))
            return rc, out.value, rt.mwhip_last_error().decode()

        for args, word in (
                ((None, 16, 8, 0, 1, [key]), "src == NULL"),
                ((ptr + 2, 15, 8, 0, 1, [key]), "multiples of 4"),
                ((ptr, 8, 10, 0, 1, [key]), "multiples of 4"),
                ((ptr, 8, 12, 2, 1, [key]), "multiples of 4"),
                ((ptr, 16, 8, 0, 0, [key]), "handles_per_record == 0"),
                ((ptr, 8, 16, 4, 2, [key]), "do not fit"),
                ((ptr, 16, 8, 4, 1, [key]), "do not fit"),
                ((ptr, 0, 8, 0, 1, [key]), "num_records == 0"),
                ((ptr, 2 ** 31, 8, 0, 1, [key]), "more than 2147483647 handles"),
                ((ptr, 2 ** 30, 16, 0, 2, [key]), "more than 2147483647 handles"),
                ((ptr, 16, 8, 0, 1, [key] * 33), "at most 32"),
                ((ptr, 16, 8, 0, 1, [key, 60000]), "component 60000 is not registered"),
                ((ptr, 16, 8, 0, 1, [key, wide, key]), "component %d is listed twice" % key),
                ((ptr, 16, 8, 0, 1, []), "n == 0"),
                ((ptr, 16, 8, 0, 1, [key, 0]), "Entity component"),
                ((ptr, 16, 8, 0, 1, [1, key]), "WorldID component"),
                # (2^31 - 1 handles x 240 bytes would be -10, below, had anything
                # been allocated before the refusal)
                ((ptr, 2 ** 31 - 1, 8, 0, 1, [wide, 0]), "Entity component"),
                ((ptr, 2 ** 31 - 1, 8, 0, 1, [wide, key, wide]), "listed twice"),
                ((ptr, 2 ** 31 - 1, 8, 0, 1, []), "n == 0")):
            rc, out, message = create(*args)
            assert rc == -2 and out == 99 and word in message, (args[1:5], rc, out, message)
            assert message.startswith("scatter_create:"), message
        # 2^31 - 1 handles x 240 bytes: more than any device has
        rc, out, message = create(ptr, 2 ** 31 - 1, 8, 0, 1, [wide])
        assert rc == -10 and out == 99 and "no device memory" in message, (rc, out, message)

        # handles: unknown, destroyed, another executor's
        rc, handle, message = create(ptr, 16, 8, 0, 1, [key])
        assert rc == 0 and handle not in (0, 99), message
        assert rt.mwhip_scatter_apply(exec_, handle) == 0
        for fn in (rt.mwhip_scatter_select, rt.mwhip_scatter_archetypes, rt.mwhip_scatter_worlds,
                   rt.mwhip_scatter_written):
            assert fn(exec_, handle)
        nbytes, cell = C.c_uint64(5), C.c_uint32(5)
        assert rt.mwhip_scatter_buffer(exec_, handle, 0, C.byref(nbytes), C.byref(cell))
        assert (nbytes.value, cell.value) == (16 * 4, 4)
        nbytes, cell = C.c_uint64(5), C.c_uint32(5)
        assert rt.mwhip_scatter_buffer(exec_, handle, 1, C.byref(nbytes), C.byref(cell)) is None
        assert "column 1 of 1" in rt.mwhip_last_error().decode()
        assert (nbytes.value, cell.value) == (5, 5)
        assert rt.mwhip_scatter_apply(other.hip_exec(), handle) == -3
        assert "scatter %d is not one of this executor's" % handle in \
            rt.mwhip_last_error().decode()
        rt.mwhip_scatter_destroy(exec_, handle)
        for call in (lambda: rt.mwhip_scatter_apply(exec_, handle),
                     lambda: rt.mwhip_scatter_apply_async(exec_, handle),
                     lambda: rt.mwhip_set_step_scatter(exec_, handle, 1)):
            assert call() == -3
            assert "scatter %d is not one of this executor's" % handle in \
                rt.mwhip_last_error().decode()
        assert rt.mwhip_scatter_buffer(exec_, handle, 0, None, None) is None
        assert rt.mwhip_scatter_written(exec_, handle) is None

        # the Python wrapper's own checks
        for source, error in ((buf.cpu(), TypeError), (buf.view(torch.int32).reshape(-1), TypeError),
                              (buf.float(), TypeError), (buf[::2], ValueError)):
            with pytest.raises(error):
                s.entity_scatter(source, ["Key"])
        for components, error in ((["Nope"], KeyError), (["Item.Key"], KeyError),
                                  (["Key", "Key"], ValueError), ([], RuntimeError),
                                  (["Entity"], RuntimeError), (["Key", "WorldID"], RuntimeError)):
            with pytest.raises(error):
                s.entity_scatter(buf, components)
        assert s._scatters == []
