"""-m gpu: state digests (mwhip_digest_*, Simulator.digest()).

The yardstick is madrona_amd/digest_ref.py, the definition in numpy, evaluated
over what the simulator dumps: the device's D[groups, worlds] must equal it bit
for bit.  Shapes are the smallest at which the kernel can still go wrong: cells
of every width it reads differently (1, 2, 4, 8, 12, 16, 20 and 240 bytes), a
world whose rows straddle a 256-row block, several worlds inside one
wavefront, one world that takes every add, tables with holes and an unsorted
tail, empty tables and empty worlds.
"""
import ctypes as C
import os

import numpy as np
import pytest

from madrona_amd import digest_ref
from madrona_amd.simlib import (DigestColumn, RING_ON_STEP, Simulator, hip_lib_path,
                                ref_lib_path, runtime_lib)

pytestmark = pytest.mark.gpu

CHURN_ONLY = 1      # sort_stress: churn without the compaction behind it


def _need_ref(sim):
    if not os.path.exists(ref_lib_path(sim)):
        pytest.skip("oracle/_ref missing on this box")


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _indices(sim, columns):
    names = [c[0] for c in sim.columns]
    if columns is None:
        return list(range(len(names)))
    return [names.index(c) if isinstance(c, str) else c for c in columns]


def _numpy_digest(sim, columns=None):
    """digest_ref over the simulator's dump (rows grouped by world)."""
    idx = _indices(sim, columns)
    tables = [sim.columns[i][0].split(".", 1)[0] for i in idx]
    return digest_ref.digest_of_dump(tables, [sim.dump_column(i, 512) for i in idx],
                                     sim.num_worlds)


def _same(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "first (group, world) that differ:", bad[:4].tolist(),
                           [hex(int(got[tuple(b)])) for b in bad[:2]],
                           [hex(int(want[tuple(b)])) for b in bad[:2]])


def _sort_stress(worlds=33, seed=7, flags=0):
    return Simulator(hip_lib_path("sort_stress"), worlds, seed=seed, flags=flags)


# ---- 1. against numpy, every width -------------------------------------------------
def test_every_cell_width_against_numpy(built):
    with _sort_stress() as s, s.digest() as dig:
        widths = {c[1] for c in s.columns if c[0].startswith("Item.")}
        assert {1, 2, 4, 8, 12, 16, 20} <= widths and max(widths) > 64, widths
        assert "Item.WorldID" in [c[0] for c in s.columns]
        assert dig.groups == ["Item", "Scratch"]
        straddles = three_in_a_wave = False
        steps = 0
        for until in (0, 1, 7):
            s.step(until - steps)
            steps = until
            D = dig.compute()
            _same(D, _numpy_digest(s), ("step", until))
            assert D[0].any()
            # the cases this shape is there for, from the dumped counts (after a
            # step the table is grouped by world in world order)
            counts = s.dump_all()["Item.Key"][1].astype(np.int64)
            ends = np.cumsum(counts)
            starts = ends - counts
            straddles |= bool(((counts > 0) & (starts // 256 != (ends - 1) // 256)).any())
            world_of_row = np.repeat(np.arange(s.num_worlds), counts)
            three_in_a_wave |= any(
                len(np.unique(world_of_row[at:at + 64])) >= 3
                for at in range(0, len(world_of_row), 64))
        assert straddles, "no world's Item rows straddle a 256-row block boundary"
        assert three_in_a_wave, "no 64-row stretch of Item holds rows of 3 worlds"


# ---- 2. unsorted table with holes ---------------------------------------------------
def test_unsorted_table_with_holes(built):
    with _sort_stress() as s:
        names = [c[0] for c in s.columns]
        item = [i for i, n in enumerate(names) if n.startswith("Item.")]
        with s.digest(item) as dig:
            s.step(4)
            cap = s.num_worlds * 80 * 4
            saw_hole = saw_unsorted = False
            for rnd in range(3):
                s.run_taskgraph(CHURN_ONLY)
                raw = [s.dump_column_raw(i, cap) for i in item]
                world = raw[item.index(names.index("Item.WorldID"))].view(np.int32).ravel()
                assert all(len(c) == len(world) for c in raw)
                saw_hole |= bool((world == -1).any())
                saw_unsorted |= bool((np.diff(world) < 0).any())
                want = digest_ref.group_digest(0, list(enumerate(raw)), world, s.num_worlds)
                _same(dig.compute(), want[None, :], ("churn", rnd))
            assert saw_hole, "no destroyed row (WorldID -1) in the raw table"
            assert saw_unsorted, "the raw world ids are non-decreasing"
            # (this is the state dump_column refuses)
            s.step(1)
            _same(dig.compute(), _numpy_digest(s, item), "after the next full step")


# ---- 3. edges -----------------------------------------------------------------------
def test_one_world(built):
    with _sort_stress(worlds=1) as s, s.digest() as dig:
        for _ in range(3):
            _same(dig.compute(), _numpy_digest(s), "1 world")
            s.step(2)


def test_one_world_with_many_rows(built, monkeypatch):
    """Every add of every wavefront lands on one address (the simulator's
    largest world: 164 rigid bodies, three wavefronts)."""
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CANDIDATES_PER_WORLD", "4096")
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CONTACTS_PER_WORLD", "1024")
    with Simulator(hip_lib_path("ball_pit"), 1, flags=150 << 16) as s, s.digest() as dig:
        rows = max(int(counts.sum()) for _, counts in s.dump_all(512).values())
        assert rows > 128, rows
        _same(dig.compute(), _numpy_digest(s), "ball_pit, start")
        s.step(1)
        _same(dig.compute(), _numpy_digest(s), "ball_pit, 1 step")


def test_plans_of_one_byte_and_interleaved_groups(built):
    with _sort_stress() as s:
        s.step(3)
        with s.digest(["Item.Tag8"]) as dig:
            assert s.columns[_indices(s, ["Item.Tag8"])[0]][1] == 1
            _same(dig.compute(), _numpy_digest(s, ["Item.Tag8"]), "one 1-byte column")
        plan = ["Scratch.Vec3", "Item.Half", "Scratch.Key", "Item.Blob20", "Item.Entity"]
        with s.digest(plan) as dig:
            assert dig.groups == ["Scratch", "Item"]
            want = _numpy_digest(s, plan)
            _same(dig.compute(), want, "interleaved")
            # the tags are plan positions: the same columns in another order hash
            # differently
            with s.digest(plan[::-1]) as other:
                assert other.groups == ["Item", "Scratch"]
                D = other.compute()
                _same(D, _numpy_digest(s, plan[::-1]), "interleaved, reversed")
                assert not np.array_equal(D[::-1], want)


def test_empty_table_and_empty_world(built):
    with _sort_stress() as s, s.digest() as dig:
        # before the first step the temporaries hold nothing
        assert s.dump_all()["Scratch.Key"][1].sum() == 0
        D = dig.compute()
        _same(D, _numpy_digest(s), "zero rows")
        assert not D[1].any()
        empty_world = False
        for step in range(1, 4):
            s.step(1)
            counts = s.dump_all()["Item.Key"][1]
            D = dig.compute()
            _same(D, _numpy_digest(s), ("step", step))
            for w in np.flatnonzero(counts == 0):
                empty_world = True
                assert D[0, w] == 0
        assert empty_world, "no world without Item rows"


# ---- 4. lock step with the reference ------------------------------------------------
def _written_before_the_first_step(name):
    """The observation outputs are first written by the first step: until then
    the reference backend holds whatever its allocator left there (heap
    addresses, stray strings: two instances of the REFERENCE differ in them, in
    every row, which is why the parity tests start comparing after step 1)."""
    column = name.split(".", 1)[1]
    return "Observation" not in column and column != "Lidar"


@pytest.mark.parametrize("sim,worlds,flags", [("cartpole", 64, 0), ("escape_room", 16, 20),
                                              ("escape_room_phys", 8, 15), ("hideseek", 8, 15)])
def test_lock_step_with_the_reference(built, sim, worlds, flags):
    """hip.digest().compute() == ref.digest().compute() at steps 0, 1 and 10.
    At step 0 the comparison with the reference is over the columns that exist
    by then (everything but the observation outputs, see above: measured on
    the MI355X box, escape_room / escape_room_phys / hideseek, the reference's
    SelfObservation, PartnerObservation, RoomEntityObservations,
    DoorObservation, AgentObservations, BoxObservations, RampObservations and
    Lidar differ between two runs of the reference itself in 36-40 of 40
    rows); the full dump list is held against numpy over the HIP side's own
    dump there, and against the reference from step 1 on."""
    _need_ref(sim)
    with Simulator(ref_lib_path(sim), worlds, seed=5, num_workers=1, flags=flags) as ref, \
            Simulator(hip_lib_path(sim), worlds, seed=5, flags=flags) as hip:
        assert ref.columns == hip.columns
        defined = [c[0] for c in hip.columns if _written_before_the_first_step(c[0])]
        assert len(defined) >= len(hip.columns) - 5 and "Observation" not in "".join(defined)
        with ref.digest() as dr, hip.digest() as dh:
            assert dr.groups == dh.groups
            with ref.digest(defined) as dr0, hip.digest(defined) as dh0:
                _same(dh0.compute(), dr0.compute(), (sim, "step", 0))
            start = dh.compute()
            _same(start, _numpy_digest(hip), (sim, "step", 0, "full list"))
            ref.step(1)
            hip.step(1)
            _same(dh.compute(), dr.compute(), (sim, "step", 1))
            ref.step(9)
            hip.step(9)
            D = dh.compute()
            _same(D, dr.compute(), (sim, "step", 10))
            assert not np.array_equal(start, D)


# ---- 5. locality --------------------------------------------------------------------
def test_one_flipped_bit_changes_one_entry(built):
    W, world = 16, 5
    with Simulator(hip_lib_path("escape_room"), W, seed=5, flags=20) as s, s.digest() as dig:
        s.step(2)
        before = dig.compute()
        action = s.read_tensor("action")
        flipped = action.copy()
        flipped[world, 1, 2] ^= 1 << 9
        s.write_tensor("action", flipped)
        after = dig.compute()
        changed = np.argwhere(after != before)
        assert changed.tolist() == [[dig.groups.index("Agent"), world]], changed
        _same(after, _numpy_digest(s), "flipped")
        s.write_tensor("action", action)
        _same(dig.compute(), before, "written back")


# ---- 6. twin side and growth --------------------------------------------------------
def _archetype_of(sim, column):
    arch, comp = C.c_uint32(0), C.c_uint32(0)
    assert sim.lib.sim_hip_column_ids(sim.handle, _indices(sim, [column])[0],
                                      C.byref(arch), C.byref(comp)) == 0
    return arch.value


def test_twin_side(built):
    """The sort that copies the rows into the columns' twins swaps the sides."""
    with _sort_stress() as s, s.digest() as dig:
        s.step(2)
        item = _archetype_of(s, "Item.Key")
        _same(dig.compute(), _numpy_digest(s), "before")
        stats = s.sort_stats()[item]
        s.step(1)
        now = s.sort_stats()[item]
        assert now["runs"] - now["stay_runs"] > stats["runs"] - stats["stay_runs"], \
            "no sort copied Item into its twin columns"
        _same(dig.compute(), _numpy_digest(s), "after")


def test_growth(built, monkeypatch):
    """The digest object is made before the tables grow."""
    monkeypatch.setenv("MADRONA_MWHIP_INITIAL_CAPACITY_DIV", "4")
    rt = runtime_lib()
    rt.mwhip_num_table_growths.restype = C.c_uint32
    rt.mwhip_num_table_growths.argtypes = [C.c_void_p]
    with _sort_stress(worlds=300, flags=2) as s, s.digest() as dig:
        s.step(3)
        _same(dig.compute(), _numpy_digest(s), "before the growth")
        grown = rt.mwhip_num_table_growths(s.hip_exec())
        s.step(37)
        assert rt.mwhip_num_table_growths(s.hip_exec()) > grown, "nothing grew"
        _same(dig.compute(), _numpy_digest(s), "after the growth")


# ---- 7. snapshot --------------------------------------------------------------------
def test_restore_puts_every_world_back(built):
    with _sort_stress() as s, s.digest() as dig:
        s.step(3)
        snap = s.snapshot()
        snap.save()
        at_save = dig.compute()
        s.step(5)
        later = dig.compute()
        assert (later[0] != at_save[0]).sum() > s.num_worlds // 2
        snap.restore()
        _same(dig.compute(), at_save, "restored")
        _same(at_save, _numpy_digest(s), "restored, against numpy")
        snap.close()


# ---- 8. stream order ----------------------------------------------------------------
def test_compute_async_is_stream_ordered(built):
    with _sort_stress() as s, _sort_stress() as twin, s.digest() as dig:
        s.step_async(3)
        dig.compute_async()
        s.step_async(3)
        s.sync()
        twin.step(3)
        want = _numpy_digest(twin)
        _same(dig.read(), want, "queued between two runs of three steps")
        twin.step(3)
        assert not np.array_equal(_numpy_digest(twin), want)
        _same(dig.compute(), _numpy_digest(twin), "six steps")


# ---- 9. step digest and ring --------------------------------------------------------
def _action(worlds, t):
    rng = np.random.default_rng([77, t])
    shape = (worlds, 2)
    return np.stack([rng.integers(0, 4, shape), rng.integers(0, 8, shape),
                     rng.integers(-2, 3, shape), np.zeros(shape, int)], -1).astype(np.int32)


def test_step_digest_recorded_by_an_output_ring(built):
    torch = _torch()
    W, K, SLOTS = 7, 6, 4
    rt = runtime_lib()
    with Simulator(hip_lib_path("escape_room"), W, seed=5, flags=20) as s, \
            Simulator(hip_lib_path("escape_room"), W, seed=5, flags=20) as twin, \
            s.digest() as dig, twin.digest() as twin_dig:
        actions = [_action(W, t) for t in range(K)]
        action_ring = torch.from_numpy(np.stack(actions)).cuda()
        groups = len(dig.groups)
        ring = torch.zeros((SLOTS, groups, W), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        s.set_input_ring("action", action_ring.data_ptr(), K)
        dig.every_step()
        assert rt.mwhip_set_output_ring(s.hip_exec(), dig.buffer_ptr, ring.data_ptr(),
                                        groups * W * 8, SLOTS, RING_ON_STEP) == 0
        s.step_async(K)
        want = []
        for k in range(K):
            twin.write_tensor("action", actions[k])
            twin.step(1)
            want.append(twin_dig.compute())
            _same(want[k], _numpy_digest(twin), ("twin", k))
        s.sync()
        recorded = ring.cpu().numpy().view(np.uint64)
        for k in range(K - SLOTS, K):       # (steps 0 and 1 were overwritten)
            _same(recorded[k % SLOTS], want[k], ("slot of step", k))
        assert not np.array_equal(want[K - 1], want[K - 2])
        # the buffer itself holds the last step's
        _same(dig.read(), want[K - 1], "the buffer after the last step")
        assert rt.mwhip_set_output_ring(s.hip_exec(), dig.buffer_ptr, None, 0, 0,
                                        RING_ON_STEP) == 0
        dig.every_step(False)
        s.set_input_ring("action", 0, K)


def test_step_digest_in_the_launch_lists(built):
    """Roles from mwhip_profile before, during and after; the packed step graph
    carries the launches in front of its pack node, the render graph has none."""
    torch = _torch()
    W, res = 2, 16
    with Simulator(hip_lib_path("escape_room_render"), W, seed=4,
                   flags=40 | (res << 16)) as s, s.digest() as dig:
        s.step(2)
        names = lambda graph=0: [k["name"] for k in s.profile(1, graph=graph)]   # noqa: E731
        before = names()
        assert not [n for n in before if "digest" in n]
        render_before = names(s.render_graph())

        dig.every_step()
        stats = s.profile(1)
        during = [k["name"] for k in stats]
        at = during.index("digest:digest.zero")
        assert during[at + 1] == "digest:digest"
        # behind every task-graph node, in front of the replay's health kernel
        assert during[:at] + during[at + 2:] == before and at == len(before) - 1
        # algo_bytes: the listed cells of the live rows (what was just hashed is
        # the state this step left)
        cell_bytes = sum(int(counts.sum()) * rows.shape[1]
                         for rows, counts in (s.dump_column(i, 512)
                                              for i in range(len(s.columns))))
        assert stats[at + 1]["algo_bytes"] == cell_bytes, (stats[at + 1], cell_bytes)
        _same(dig.read(), _numpy_digest(s), "what the profiled step left in the buffer")

        packed_dst = torch.zeros((W, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        packed = s.packed_step_graph(["reward", "done"], packed_dst.data_ptr())
        in_packed = names(packed)
        assert in_packed.index("digest:digest.zero") + 1 == in_packed.index("digest:digest") \
            == in_packed.index("pack:pack.rows") - 1, in_packed
        s.step_async(1, graph=packed)
        s.sync()
        _same(dig.read(), _numpy_digest(s), "a replay of the packed graph")
        assert names(s.render_graph()) == render_before

        dig.every_step(False)
        assert names() == before
        assert "digest:digest" not in names(packed)


# ---- 10. refusals at the ABI --------------------------------------------------------
def test_refusals(built):
    rt = runtime_lib()
    with _sort_stress(worlds=3) as s:
        keeper = s.digest()
        s.step(1)
        exec_ = s.hip_exec()
        item, scratch = _archetype_of(s, "Item.Key"), _archetype_of(s, "Scratch.Key")
        comp = {}
        for name in ("Item.Key", "Item.Wide"):
            a, c = C.c_uint32(0), C.c_uint32(0)
            s.lib.sim_hip_column_ids(s.handle, _indices(s, [name])[0], C.byref(a), C.byref(c))
            comp[name] = c.value
        want = keeper.compute()

        def create(pairs, n=None):
            plan = (DigestColumn * max(len(pairs), 1))(*[DigestColumn(a, c) for a, c in pairs])
            out = C.c_uint64(99)
            rc = rt.mwhip_digest_create(exec_, plan, len(pairs) if n is None else n,
                                        C.byref(out))
            return rc, out.value, rt.mwhip_last_error().decode()

        cap = 256       # MWHIP_DIGEST_MAX_COLUMNS
        for pairs, n, word in (
                ([(item, 0)], 0, "n == 0"),
                ([(item, 0), (250, 0)], None, "archetype 250"),
                ([(scratch, comp["Item.Wide"])], None, "no component"),
                ([(item, comp["Item.Key"]), (item, 1), (item, comp["Item.Key"])], None, "twice"),
                ([(item, 0)] * (cap + 1), None, "at most %d" % cap)):
            rc, out, message = create(pairs, n)
            assert rc != 0 and out == 99 and word in message, (pairs[:3], rc, out, message)

        rc, handle, message = create([(item, comp["Item.Key"])])
        assert rc == 0 and handle not in (0, 99), message
        assert rt.mwhip_digest_compute(exec_, handle) == 0
        rt.mwhip_digest_destroy(exec_, handle)
        for call in (rt.mwhip_digest_compute, rt.mwhip_digest_compute_async,
                     rt.mwhip_set_step_digest):
            assert call(exec_, handle) != 0
            assert "digest %d is not one of this executor's" % handle in \
                rt.mwhip_last_error().decode()
        assert rt.mwhip_digest_buffer(exec_, handle, None, None) is None
        # nothing changed for the digest that was there all along
        _same(keeper.compute(), want, "after the refusals")
    # Simulator.close() orphaned it
    try:
        keeper.compute()
    except RuntimeError as err:
        assert "closed" in str(err)
    else:
        raise AssertionError("a digest outlived its simulator")
