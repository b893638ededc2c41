"""GPU: entity gathers (mwhip_gather_*, Simulator.entity_gather, csrc/entity_gather.hip)
against madrona_amd/gather_ref.py over table-order dumps of EVERY registered
table of the executor (mwhip_dump_column_raw, what Simulator.dump_column_raw
calls, asked for the Entity and WorldID columns of tables the dump list does not
show too): every byte of every buffer and both int32 outputs."""
import ctypes as C
import os

import numpy as np
import pytest

from madrona_amd.gather_ref import gather_ref, read_handles, table_of_dump, table_of_raw
from madrona_amd.simlib import (RING_ON_STEP, GatherSource, Simulator, hip_lib_path,
                                ref_lib_path, runtime_lib)

pytestmark = pytest.mark.gpu

CHURN_ONLY = 1      # sort_stress: churn without the compaction behind it
SORT_BY_KEY = 2     # sort_stress: a sort of Item by Key (no world-sorted prefix is left)
COMPACT_ONLY = 3    # sort_stress: the compaction that has to follow it
RAW_CAP = 1 << 16   # rows a table-order dump has room for
MAX_ARCHETYPES = 256
NONE = (0xFFFFFFFF, 0xFFFFFFFF)     # Entity::none()


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


def _components(sim, names):
    """[(name, component id, cell bytes)] of components named as entity_gather names them"""
    out = []
    for name in names:
        column = next(c for c in sim.columns if c[0].split(".", 1)[1] == name)
        out.append((name, _ids(sim, column[0])[1], column[1]))
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


def _tables(sim, names):
    """Every registered table of the executor with its Entity and WorldID
    columns and those of `names` it has, in table order."""
    rt = _rt()
    comps = _components(sim, names)
    tables = []
    for a in range(MAX_ARCHETYPES):
        if rt.mwhip_num_rows(sim.hip_exec(), a) < 0:
            continue
        columns = {}
        for name, comp, cell in comps:
            cells = _raw(sim, a, comp, cell)
            if cells is not None:
                columns[name] = cells
        tables.append(table_of_raw(a, _raw(sim, a, 0, 8), _raw(sim, a, 1, 4), columns))
    return tables


def _got(gather):
    gather._sim.sync()
    return (gather.archetypes.cpu().numpy(), gather.worlds.cpu().numpy(),
            {name: gather.tensor(name).cpu().numpy() for name in gather.components})


def _same(got, want, what):
    for k, label in ((0, "archetype"), (1, "world")):
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, (what, label)
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, (what, label, "differs at handles", bad[:4].tolist(),
                               got[k][bad[:4]].tolist(), want[k][bad[:4]].tolist())
    assert list(got[2]) == list(want[2])
    for name, want_bytes in want[2].items():
        got_bytes = got[2][name]
        assert got_bytes.dtype == np.uint8 and got_bytes.shape == want_bytes.shape, \
            (what, name, got_bytes.shape, want_bytes.shape)
        bad = np.argwhere(got_bytes != want_bytes)
        assert len(bad) == 0, (what, name, len(bad), "bytes differ, first (handle, byte):",
                               bad[:4].tolist())


def _check(sim, gather, handles, what):
    """compute, then compare with gather_ref of `handles` (uint32 [N, 2])"""
    gather.compute()
    comps = [(n, gather.cell_bytes(n)) for n in gather.components]
    want = gather_ref(handles, _tables(sim, gather.components), comps)
    assert len(handles) == gather.num_handles
    _same(_got(gather), want, what)
    return want


def _slab_handles(view, name, first_byte=0, handles=1):
    """the handles a gather over view.handle_source(...) reads, from the slab"""
    view.compute()
    ptr, records, record_bytes, first, per = view.handle_source(name, first_byte, handles)
    return read_handles(view.tensor(name).cpu().numpy(), records, record_bytes, first, per)


def _device_handles(handles):
    """uint32 [N, 2] as a torch int32 [N, 2] on the device"""
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(handles).view(np.int32).copy()).cuda()


def _live_set(tables):
    """({(gen, id)} of the live rows that hold an entity, {id: gen}) over every
    table (a temporary's row and a destroyed one hold Entity::none(), id -1)"""
    live, gens = set(), {}
    for t in tables:
        for (gen, ident), w in zip(t.entities.tolist(), t.world_ids.tolist()):
            if w != -1 and ident < 2 ** 31:
                live.add((gen, ident))
                gens[ident] = gen
    return live, gens


ITEM = ["Entity", "Tag8", "Half", "Key", "Pair", "Vec3", "Quad", "Blob20", "Wide", "WorldID"]


# ---- 1. widths, teams, partial last wave --------------------------------------------
def test_every_cell_width_team_size_and_a_partial_last_wave(built):
    torch = _torch()
    with _sort_stress() as s, s.world_view("Item", ["Item.Entity"], max_rows=40) as hv, \
            s.world_view("Item", max_rows=40) as full, \
            s.entity_gather(hv.handle_source("Item.Entity"), ITEM) as g:
        assert g.num_handles == 33 * 40 == 1320 and g.num_handles % 64 != 0
        widths = sorted(g.cell_bytes(n) for n in ITEM)
        assert widths == [1, 2, 4, 4, 8, 8, 12, 16, 20, 240], widths
        steps = 0
        for until in (0, 1, 7):
            s.step(until - steps)
            steps = until
            handles = _slab_handles(hv, "Item.Entity")
            # every byte of every output is rewritten by every compute
            for name in ITEM:
                g.tensor(name).fill_(0xFF)
            g.archetypes.fill_(77)
            g.worlds.fill_(77)
            torch.cuda.synchronize()
            archetype, world, cells = _check(s, g, handles, ("step", until))
            item = _ids(s, "Item.Key")[0]
            counts = full.compute().counts.cpu().numpy()
            assert counts.max() <= 40 and 0 < counts.sum() < 1320
            rank = np.tile(np.arange(40), 33)
            in_table = rank < np.repeat(counts, 40)
            # the handles of a world's rows name those rows; the zero padding is
            # a handle too, whatever it names
            assert (archetype[in_table] == item).all()
            assert (world[in_table] == np.repeat(np.arange(33), 40)[in_table]).all()
            got = _got(g)[2]
            for name in ITEM:
                view_cells = full.tensor("Item." + name).cpu().numpy().reshape(1320, -1)
                assert np.array_equal(got[name][in_table], view_cells[in_table]), (until, name)
        # typed tensors over the same bytes
        vec3 = g.tensor("Vec3", np.float32)
        assert tuple(vec3.shape) == (1320, 3)
        assert np.array_equal(vec3.cpu().numpy().view(np.uint8).reshape(1320, 12), got["Vec3"])


# ---- 2. stale and reused handles ----------------------------------------------------
def test_stale_and_reused_handles(built):
    """The handles of step 2, looked up at step 7.  The reference CPU backend's
    sort_stress (33 worlds, seed 7), whose entity ids are this backend's, by its
    Item.Entity dump: of the 632 handles live at step 2, 302 are still live at
    step 7, 263 have their id held with another generation, 67 have a free id
    (Scratch rows may hold a few of those).  The zero padding of the slab makes
    1320 handles."""
    with _sort_stress() as s, s.world_view("Item", ["Item.Entity"], max_rows=40) as hv:
        s.step(2)
        handles = _slab_handles(hv, "Item.Entity")
        counts = hv.counts.cpu().numpy()
        kept = _device_handles(handles)
        with s.entity_gather(kept, ITEM) as g:
            _check(s, g, handles, "at step 2")
            s.step(5)
            archetype, world, cells = _check(s, g, handles, "at step 7")
            live, gens = _live_set(_tables(s, []))
            in_table = np.tile(np.arange(40), 33) < np.repeat(counts, 40)
            real = [tuple(h) for h in handles[in_table].tolist()]
            assert len(real) == 632
            still = sum(h in live for h in real)
            regenerated = sum(h not in live and h[1] in gens for h in real)
            free = sum(h[1] not in gens for h in real)
            print("still live", still, "other generation", regenerated, "free id", free)
            assert still >= 1 and regenerated >= 1 and free >= 1
            assert still + regenerated + free == 632
            named = int((archetype >= 0).sum())
            assert still <= named <= still + (1320 - 632)
            assert not cells["Wide"][archetype < 0].any()


# ---- 3. any archetype, absent components, handles that name nothing ----------------
def test_any_archetype_absent_components_and_handles_that_name_nothing(built):
    """Handles of Item, of Scratch and of Reuse0 .. Reuse4 (flags 128) in one
    list.  Scratch rows are temporaries (makeTemporary): their Entity cells hold
    Entity::none(), so "the handles of Scratch" are that many handles that name
    nothing, although cells hold them; the Reuse tables (Key, Pair) are the other
    archetypes whose rows get zero Vec3 and Wide."""
    torch = _torch()
    with _sort_stress(flags=128) as s:
        s.step(3)
        item, scratch = _ids(s, "Item.Key")[0], _ids(s, "Scratch.Key")[0]
        reuse = [_ids(s, "Reuse%d.Key" % k)[0] for k in range(5)]
        tables = {t.archetype: t for t in _tables(s, [])}
        item_handles = tables[item].entities
        scratch_handles = tables[scratch].entities
        reuse_handles = np.concatenate([tables[a].entities for a in reuse])
        reuse_of = np.concatenate([np.full(len(tables[a].entities), a) for a in reuse])
        assert len(item_handles) > 64 and len(scratch_handles) > 64 and len(reuse_handles) > 64
        assert sum(len(tables[a].entities) > 0 for a in reuse) >= 3
        for a in [item, scratch] + reuse:
            assert (tables[a].world_ids >= 0).all()
        assert (scratch_handles == np.array(NONE, dtype=np.uint32)).all()
        live, gens = _live_set(tables.values())
        past = (max(gens) // 64 + 1) * 64       # rounded up past every id in use
        live_gen, live_id = (int(v) for v in item_handles[5])
        assert (live_gen, live_id) in live and live_gen != 0xFFFFFFFF, (live_gen, live_id)
        extras = np.array([NONE, (0, 0), (0, 2 ** 31 - 1), (0, 0xFFFFFFFE),      # (id -2)
                           (0, past), ((live_gen + 1) & 0xFFFFFFFF, live_id)], dtype=np.uint32)
        handles = np.concatenate([item_handles, scratch_handles, reuse_handles, extras])
        kept = _device_handles(handles)
        names = ["Key", "Pair", "Vec3", "Wide"]
        with s.entity_gather(kept, names) as g:
            archetype, world, cells = _check(s, g, handles, "Item + Scratch + Reuse + extras")
            ni, ns, nr = len(item_handles), len(scratch_handles), len(reuse_handles)
            assert (archetype[:ni] == item).all()
            assert (archetype[ni:ni + ns] == -1).all()
            assert np.array_equal(archetype[ni + ns:ni + ns + nr], reuse_of)
            assert cells["Wide"][:ni].any() and cells["Vec3"][:ni].any()
            rows = slice(ni + ns, ni + ns + nr)
            assert cells["Key"][rows].any() and cells["Pair"][rows].any()
            assert not cells["Wide"][rows].any() and not cells["Vec3"][rows].any()
            at = ni + ns + nr
            for k in (0, 2, 3, 4, 5):
                assert archetype[at + k] == -1 and world[at + k] == -1, extras[k]
            # the same handles as uint8 [N, 8], and (where torch has it) uint32 [N, 2]
            forms = [kept.view(torch.uint8).reshape(-1, 8)]
            if hasattr(torch, "uint32"):
                forms.append(kept.view(torch.uint32))
            for form in forms:
                with s.entity_gather(form, names) as other:
                    other.compute()
                    _same(_got(other), (archetype, world, cells), str(form.dtype))
        # no components: archetypes and worlds alone
        with s.entity_gather(kept, []) as bare:
            want = _check(s, bare, handles, "n == 0")
            assert want[2] == {} and np.array_equal(want[0], archetype)


# ---- 4. tables that are not sorted --------------------------------------------------
def test_unsorted_tables_and_the_twin_swap(built):
    """One gather object over three graphs: churn without compaction (holes,
    rows behind the prefix), a sort by key (no prefix; the columns swap with
    their twins) and the compaction after it (they swap again)."""
    with _sort_stress() as s, s.world_view("Item", ["Item.Entity"], max_rows=40) as hv:
        s.step(4)
        before = _slab_handles(hv, "Item.Entity")
        kept = _device_handles(before)
        with s.entity_gather(hv.handle_source("Item.Entity"), ITEM) as fresh, \
                s.entity_gather(kept, ["Key", "Wide", "Tag8"]) as old:
            saw_destroyed = saw_tail = False
            for what, graph in (("churn 0", CHURN_ONLY), ("churn 1", CHURN_ONLY),
                                ("sorted by key", SORT_BY_KEY), ("compacted", COMPACT_ONLY)):
                s.run_taskgraph(graph)
                _check(s, fresh, _slab_handles(hv, "Item.Entity"), ("fresh", what))
                archetype, _, _ = _check(s, old, before, ("old", what))
                item = next(t for t in _tables(s, []) if t.archetype == _ids(s, "Item.Key")[0])
                if what.startswith("churn"):
                    # rows destroyed in place stay where they are (WorldID -1,
                    # Entity::none()); the handles of step 4 that named one name
                    # nothing now
                    assert (item.world_ids == -1).any(), "no destroyed row in the raw table"
                    saw_tail |= bool((np.diff(item.world_ids) < 0).any())
                    live, _ = _live_set([item])
                    gone = [i for i, h in enumerate(before.tolist())
                            if tuple(h) != (0, 0) and tuple(h) not in live]
                    saw_destroyed |= bool(gone)
                    assert (archetype[gone] == -1).all()
                if what == "sorted by key":
                    live = item.world_ids[item.world_ids >= 0]
                    assert (np.diff(live) < 0).sum() > len(live) // 4, "the worlds stayed grouped"
            assert saw_destroyed, "no handle of step 4 named a row that was destroyed in place"
            assert saw_tail, "no row behind the sorted prefix"
            s.step(1)
            _check(s, fresh, _slab_handles(hv, "Item.Entity"), "after the next full step")
            _check(s, old, before, "old, after the next full step")


# ---- 5. growth after create ---------------------------------------------------------
def test_ids_taken_at_run_time_after_create(built):
    """Cold start: some worlds take their first block of entity ids at run time,
    behind every id handed out at init."""
    with _sort_stress(flags=1) as s, s.world_view("Item", ["Item.Entity"], max_rows=40) as hv, \
            s.entity_gather(hv.handle_source("Item.Entity"), ITEM) as g:
        _, gens = _live_set(_tables(s, []))
        # (ids are handed out in blocks of 64: no id of init lies behind this one)
        init_end = (max(gens) // 64 + 1) * 64 if gens else 0
        s.step(10)
        handles = _slab_handles(hv, "Item.Entity")
        archetype, _, _ = _check(s, g, handles, "cold start, 10 steps")
        ids = handles[:, 1].astype(np.int64)
        late = (ids >= init_end) & (archetype >= 0)
        assert late.any(), ("no live id behind the ids of init", init_end, int(ids.max()))


def test_tables_that_grew_after_create(built, monkeypatch):
    """Ramp-up: the tables grow at run time."""
    monkeypatch.setenv("MADRONA_MWHIP_INITIAL_CAPACITY_DIV", "4")
    rt = _rt()
    with _sort_stress(worlds=300, flags=2) as s, \
            s.world_view("Item", ["Item.Entity"], max_rows=40) as hv, \
            s.entity_gather(hv.handle_source("Item.Entity"), ["Key", "Vec3", "Wide", "Tag8"]) as g:
        grown = rt.mwhip_num_table_growths(s.hip_exec())
        rows = rt.mwhip_num_rows(s.hip_exec(), _ids(s, "Item.Key")[0])
        _check(s, g, _slab_handles(hv, "Item.Entity"), "before the growth")
        s.step(40)
        assert rt.mwhip_num_table_growths(s.hip_exec()) > grown, "nothing grew"
        assert rt.mwhip_num_rows(s.hip_exec(), _ids(s, "Item.Key")[0]) > 4 * rows
        archetype, _, _ = _check(s, g, _slab_handles(hv, "Item.Entity"), "after the growth")
        assert (archetype >= 0).sum() > 4 * rows


# ---- 6. two-level source ------------------------------------------------------------
def test_two_level_sources(built):
    torch = _torch()
    with Simulator(hip_lib_path("escape_room"), 5, seed=5) as s, \
            s.world_view("DoorEntity", ["DoorEntity.DoorProperties"], max_rows=4) as dv:
        s.step(3)
        assert dv.cell_bytes("DoorEntity.DoorProperties") == 40
        source = dv.handle_source("DoorEntity.DoorProperties", first_byte=0, handles=4)
        assert source[1:] == (5 * 4, 40, 0, 4)
        with s.entity_gather(source, ["Position", "ButtonState"]) as g:
            assert g.num_handles == 80
            handles = _slab_handles(dv, "DoorEntity.DoorProperties", 0, 4)
            archetype, world, cells = _check(s, g, handles, "the doors' buttons")
            button = _ids(s, "ButtonEntity.ButtonState")[0]
            props = dv.tensor("DoorEntity.DoorProperties", np.int32).cpu().numpy()
            num_buttons = props.reshape(20, 10)[:, 8]
            assert dv.counts.cpu().numpy().tolist() == [3] * 5 and num_buttons.sum() >= 15
            named = np.arange(4)[None, :] < num_buttons[:, None]
            assert (archetype.reshape(20, 4)[named] == button).all()
            assert (world.reshape(20, 4)[named] == np.repeat(np.arange(5), 4)[:, None]
                    .repeat(4, 1)[named]).all()
            assert cells["Position"].reshape(20, 4, 12)[named].any()
        for bad in ((16, 4), (0, 6), (-8, 1), (0, 0)):
            with pytest.raises(ValueError):
                dv.handle_source("DoorEntity.DoorProperties", *bad)

        # records of 24 bytes with one handle at byte 8, the rest never read as one
        tables = _tables(s, [])
        pool = np.concatenate([t.entities for t in tables if len(t.entities)])
        rng = np.random.default_rng(3)
        chosen = pool[rng.integers(0, len(pool), 150)]
        chosen[::7] = NONE
        records = np.full((150, 24), 0xCD, dtype=np.uint8)
        records[:, 8:16] = chosen.view(np.uint8).reshape(150, 8)
        buf = torch.from_numpy(records).cuda()
        with s.entity_gather((buf.data_ptr(), 150, 24, 8, 1), ["Position", "ButtonState"]) as g:
            archetype, _, _ = _check(s, g, chosen, "24-byte records")
            assert len(np.unique(archetype)) >= 4       # nothing, and three kinds of entity


# ---- 7. against the reference backend -----------------------------------------------
def test_lock_step_with_the_reference(built):
    """Position and Rotation through Agent.OtherAgents, ButtonState through the
    doors' buttons: what the HIP backend gathers equals gather_ref over the
    reference CPU backend's own dump with the reference's own handles, across
    episode resets (autoResetDenom 6: buttons are destroyed and made again)."""
    _need_ref("escape_room")
    W = 5
    rng = np.random.default_rng(0)
    with Simulator(ref_lib_path("escape_room"), W, seed=5, num_workers=1, flags=6) as ref, \
            Simulator(hip_lib_path("escape_room"), W, seed=5, flags=6) as hip, \
            hip.world_view("Agent", ["Agent.OtherAgents"], max_rows=2) as av, \
            hip.world_view("DoorEntity", ["DoorEntity.DoorProperties"], max_rows=3) as dv, \
            hip.entity_gather(av.handle_source("Agent.OtherAgents"),
                              ["Position", "Rotation"]) as agents, \
            hip.entity_gather(dv.handle_source("DoorEntity.DoorProperties", 0, 4),
                              ["ButtonState"]) as buttons:
        archetypes = {t: _ids(hip, t + ".Entity")[0]
                      for t in ("Agent", "PhysicsEntity", "DoorEntity", "ButtonEntity")}
        resets = 0
        last_remaining = None
        button_gens = set()
        for step in range(1, 13):
            a = np.stack([rng.integers(0, 4, (W, 2)), rng.integers(0, 8, (W, 2)),
                          rng.integers(-2, 3, (W, 2)), np.zeros((W, 2), int)],
                         -1).astype(np.int32)
            ref.write_tensor("action", a)
            hip.write_tensor("action", a)
            ref.step(1)
            hip.step(1)
            remaining = ref.read_tensor("steps_remaining").ravel()
            if last_remaining is not None:
                resets += int((remaining > last_remaining).sum())
            last_remaining = remaining
            if step not in (1, 2, 5, 8, 12):
                continue
            dump = ref.dump_all(512)
            tables = []
            for t, a_id in archetypes.items():
                cols = {n.split(".", 1)[1]: dump[n] for n in dump
                        if n.split(".", 1)[0] == t
                        and n.split(".", 1)[1] in ("Position", "Rotation", "ButtonState")}
                tables.append(table_of_dump(a_id, dump[t + ".Entity"], cols))
            rows, counts = dump["Agent.OtherAgents"]
            assert counts.tolist() == [2] * W
            ref_agents = read_handles(rows, 2 * W, 8)
            rows, counts = dump["DoorEntity.DoorProperties"]
            assert counts.tolist() == [3] * W
            ref_buttons = read_handles(rows, 3 * W, 40, 0, 4)
            button_gens |= set(ref_buttons[:, 0].tolist())

            av.compute()
            dv.compute()
            want = gather_ref(ref_agents, tables, [("Position", 12), ("Rotation", 16)])
            assert (want[0] == archetypes["Agent"]).all()
            _same(_got(agents.compute()), want, ("OtherAgents", step))
            want = gather_ref(ref_buttons, tables, [("ButtonState", 4)])
            assert (want[0] == archetypes["ButtonEntity"]).sum() >= 3 * W
            _same(_got(buttons.compute()), want, ("buttons", step))
        assert resets >= 1, "no episode was reset"
        assert len(button_gens - {0xFFFFFFFF}) >= 2, "no button was made again"


# ---- 8. every step, with a ring -----------------------------------------------------
def test_step_gather_over_a_step_view_recorded_by_an_output_ring(built):
    torch = _torch()
    K, W = 4, 5
    N = 2 * W
    rt = runtime_lib()
    rng = np.random.default_rng(1)
    actions = np.stack([rng.integers(1, 4, (W, 2)), rng.integers(0, 8, (W, 2)),
                        rng.integers(-2, 3, (W, 2)), np.zeros((W, 2), int)], -1).astype(np.int32)
    with Simulator(hip_lib_path("escape_room"), W, seed=5) as s, \
            Simulator(hip_lib_path("escape_room"), W, seed=5) as twin, \
            s.world_view("Agent", ["Agent.OtherAgents"], max_rows=2) as sv, \
            twin.world_view("Agent", ["Agent.OtherAgents"], max_rows=2) as tv, \
            s.entity_gather(sv.handle_source("Agent.OtherAgents"), ["Position"]) as g, \
            twin.entity_gather(tv.handle_source("Agent.OtherAgents"), ["Position"]) as tg:
        s.write_tensor("action", actions)
        twin.write_tensor("action", actions)
        names = lambda: [k["name"] for k in s.profile(1)]   # noqa: E731
        sv.every_step()
        base = names()
        twin.step(1)        # (the profiled step)
        assert base.count("view:view") == 1 and "gather:gather" not in base

        ring = torch.zeros((K, N, 12), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g.every_step()
        assert rt.mwhip_set_output_ring(s.hip_exec(), g.buffer_ptr("Position"), ring.data_ptr(),
                                        N * 12, K, RING_ON_STEP) == 0
        s.step_async(K)
        want = []
        for k in range(K):
            twin.step(1)
            want.append(_check(twin, tg, _slab_handles(tv, "Agent.OtherAgents"), ("twin", k)))
        s.sync()
        recorded = ring.cpu().numpy()
        for k in range(K):
            assert np.array_equal(recorded[k], want[k][2]["Position"]), ("slot of step", k)
        assert not np.array_equal(recorded[K - 1], recorded[0]), "nobody moved"
        # the buffers themselves hold the last step's
        _same(_got(g), want[K - 1], "the buffers after the last step")

        # one launch, directly behind the step views and in front of the ring
        stats = s.profile(1)
        during = [k["name"] for k in stats]
        at = during.index("gather:gather")
        assert during.count("gather:gather") == 1
        assert during[at - 1] == "view:view" and during[at + 1] == "ring:ring.out", during
        assert during[:at] + during[at + 2:] == base
        # algo_bytes: everything written + the handles + per named handle its
        # slot, its row's Entity and WorldID cells and its Position
        named = int((g.archetypes.cpu().numpy() >= 0).sum())
        assert named == N
        assert stats[at]["algo_bytes"] == N * (12 + 8) + N * 8 + named * (12 + 12 + 12), stats[at]

        assert rt.mwhip_set_output_ring(s.hip_exec(), g.buffer_ptr("Position"), None, 0, 0,
                                        RING_ON_STEP) == 0
        g.every_step(False)
        assert names() == base


# ---- 9. snapshot --------------------------------------------------------------------
def test_restore_then_compute_gives_the_saved_gather(built):
    with _sort_stress() as s, s.world_view("Item", ["Item.Entity"], max_rows=40) as hv:
        s.step(3)
        handles = _slab_handles(hv, "Item.Entity")
        kept = _device_handles(handles)
        with s.entity_gather(kept, ["Key", "Quad", "WorldID"]) as g, s.snapshot() as snap:
            snap.save()
            at_save = _check(s, g, handles, "at the save")
            s.step(3)
            later = _check(s, g, handles, "3 steps later")
            assert not np.array_equal(later[0], at_save[0])
            snap.restore()
            # (gathers are derived state: the buffers still hold the later one)
            _same(_got(g), later, "restored, not yet computed")
            g.compute()
            _same(_got(g), at_save, "restored and computed")


# ---- 10. refusals -------------------------------------------------------------------
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
            rc = rt.mwhip_gather_create(exec_, C.byref(source), arr,
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
                ((ptr, 16, 8, 0, 1, [key, wide, key]), "component %d is listed twice" % key)):
            rc, out, message = create(*args)
            assert rc == -2 and out == 99 and word in message, (args[1:5], rc, out, message)
        # 2^31 - 1 handles x 240 bytes: more than any device has
        rc, out, message = create(ptr, 2 ** 31 - 1, 8, 0, 1, [wide])
        assert rc == -10 and out == 99 and "no device memory" in message, (rc, out, message)

        # handles: unknown, destroyed, another executor's; n == 0 is allowed
        rc, handle, message = create(ptr, 16, 8, 0, 1, [])
        assert rc == 0 and handle not in (0, 99), message
        assert rt.mwhip_gather_compute(exec_, handle) == 0
        assert rt.mwhip_gather_archetypes(exec_, handle) and rt.mwhip_gather_worlds(exec_, handle)
        nbytes, cell = C.c_uint64(5), C.c_uint32(5)
        assert rt.mwhip_gather_buffer(exec_, handle, 0, C.byref(nbytes), C.byref(cell)) is None
        assert "column 0 of 0" in rt.mwhip_last_error().decode()
        assert (nbytes.value, cell.value) == (5, 5)
        assert rt.mwhip_gather_compute(other.hip_exec(), handle) == -3
        assert "gather %d is not one of this executor's" % handle in \
            rt.mwhip_last_error().decode()
        rt.mwhip_gather_destroy(exec_, handle)
        for call in (lambda: rt.mwhip_gather_compute(exec_, handle),
                     lambda: rt.mwhip_gather_compute_async(exec_, handle),
                     lambda: rt.mwhip_set_step_gather(exec_, handle, 1)):
            assert call() == -3
            assert "gather %d is not one of this executor's" % handle in \
                rt.mwhip_last_error().decode()
        assert rt.mwhip_gather_buffer(exec_, handle, 0, None, None) is None
        assert rt.mwhip_gather_archetypes(exec_, handle) is None

        # the Python wrapper's own checks
        for source, error in ((buf.cpu(), TypeError), (buf.view(torch.int32).reshape(-1), TypeError),
                              (buf.float(), TypeError), (buf[::2], ValueError)):
            with pytest.raises(error):
                s.entity_gather(source, ["Key"])
        for components, error in ((["Nope"], KeyError), (["Item.Key"], KeyError),
                                  (["Key", "Key"], ValueError)):
            with pytest.raises(error):
                s.entity_gather(buf, components)
        assert s._gathers == []

        # a ninth step gather; destroying a step gather unsets it
        before = [k["name"] for k in s.profile(1)]
        gathers = [s.entity_gather(buf, ["Key"]) for _ in range(9)]
        for g in gathers[:8]:
            g.every_step()
        launches = [k["name"] for k in s.profile(1)]
        assert launches.count("gather:gather") == 1, launches
        try:
            gathers[8].every_step()
        except RuntimeError as err:
            assert "-> -2" in str(err) and "at most 8" in str(err)
        else:
            raise AssertionError("a ninth step gather was taken")
        gathers[0].close()
        gathers[8].every_step()
        s.step(2)       # (the step graph replays without the one destroyed)
        for g in gathers[1:]:
            g.close()
        assert [k["name"] for k in s.profile(1)] == before
        s.step(1)
