"""CPU-only: madrona_amd/scatter_ref.py, the definition of an entity scatter, on
hand-made tables."""
import numpy as np
import pytest

from madrona_amd.gather_ref import gather_ref, table_of_raw
from madrona_amd.scatter_ref import scatter_ref

NONE = (0xFFFFFFFF, 0xFFFFFFFF)     # Entity::none(): gen 0xFFFFFFFF, id -1


def _ents(pairs):
    return np.array(pairs, dtype=np.uint32).reshape(-1, 2)


def _cells(rows, size, salt):
    return ((np.arange(rows * size).reshape(rows, size) * 7 + salt) % 251).astype(np.uint8)


def _tables():
    """Table 3 (Pos 12 bytes, Tag 1 byte): rows of worlds 0, 0, 1, one row
    destroyed in place (Entity cell still there, WorldID -1), one more of world
    1, and a temporary's row (Entity::none(), world 1).  Table 5 (Pos only): two
    rows of world 1 and 0."""
    a = table_of_raw(3, _ents([(0, 4), (2, 9), (1, 6), (0, 7), (5, 12), NONE]),
                     np.array([0, 0, 1, -1, 1, 1], np.int32),
                     {"Pos": _cells(6, 12, 1), "Tag": _cells(6, 1, 2)})
    b = table_of_raw(5, _ents([(0, 20), (3, 21)]), np.array([1, 0], np.int32),
                     {"Pos": _cells(2, 12, 3)})
    return a, b


def _inputs(n):
    return {"Pos": _cells(n, 12, 101) | 0x80, "Tag": _cells(n, 1, 55) | 0x80}


def _unchanged(before, after, except_rows):
    """every cell of every column but those of `except_rows` {(table index,
    column): rows} is as it was; Entity and WorldID too"""
    for t, (b, a) in enumerate(zip(before, after)):
        assert a.archetype == b.archetype
        assert np.array_equal(a.entities, b.entities) and np.array_equal(a.world_ids, b.world_ids)
        assert list(a.columns) == list(b.columns)
        for name in b.columns:
            keep = np.ones(len(b.world_ids), bool)
            keep[list(except_rows.get((t, name), []))] = False
            assert np.array_equal(a.columns[name][keep], b.columns[name][keep]), (t, name)


def test_the_last_selected_handle_wins():
    a, b = _tables()
    handles = _ents([(2, 9), (0, 4), (2, 9), (2, 9)])
    inputs = _inputs(4)
    archetype, world, written, after = scatter_ref(handles, [1, 1, 7, -1], [a, b], inputs)
    assert archetype.dtype == world.dtype == written.dtype == np.int32
    assert archetype.tolist() == [3, 3, 3, 3] and world.tolist() == [0, 0, 0, 0]
    assert written.tolist() == [0, 1, 0, 1]
    assert np.array_equal(after[0].columns["Pos"][1], inputs["Pos"][3])
    assert np.array_equal(after[0].columns["Tag"][1], inputs["Tag"][3])
    assert np.array_equal(after[0].columns["Pos"][0], inputs["Pos"][1])
    _unchanged([a, b], after, {(0, "Pos"): [0, 1], (0, "Tag"): [0, 1]})
    # the tables given are not modified
    fresh = _tables()
    for given, same in zip((a, b), fresh):
        for name in same.columns:
            assert np.array_equal(given.columns[name], same.columns[name])


def test_an_unselected_later_duplicate_does_not_win():
    a, b = _tables()
    handles = _ents([(2, 9), (2, 9), (2, 9)])
    inputs = _inputs(3)
    archetype, world, written, after = scatter_ref(handles, [0, 1, 0], [a, b], inputs)
    assert written.tolist() == [0, 1, 0]
    assert archetype.tolist() == [3, 3, 3]      # whatever select says
    assert np.array_equal(after[0].columns["Pos"][1], inputs["Pos"][1])
    _unchanged([a, b], after, {(0, "Pos"): [1], (0, "Tag"): [1]})


def test_nothing_selected_changes_nothing():
    a, b = _tables()
    handles = _ents([(2, 9), (0, 20)])
    archetype, world, written, after = scatter_ref(handles, [0, 0], [a, b], _inputs(2))
    assert archetype.tolist() == [3, 5] and world.tolist() == [0, 1]
    assert written.tolist() == [0, 0]
    _unchanged([a, b], after, {})


def test_handles_that_name_nothing_change_nothing():
    a, b = _tables()
    handles = _ents([NONE,          # which the temporary's row holds, too
                     (1, 9),        # a stale generation
                     (0, 7),        # the row destroyed in place (WorldID -1)
                     (0, 1000),     # an id nobody has
                     (0, 0xFFFFFFFE)])      # id -2
    archetype, world, written, after = scatter_ref(handles, np.ones(5, np.int32), [a, b],
                                                   _inputs(5))
    assert archetype.tolist() == [-1] * 5 and world.tolist() == [-1] * 5
    assert written.tolist() == [0] * 5
    _unchanged([a, b], after, {})


def test_a_table_without_the_column_still_counts_as_written():
    a, b = _tables()
    handles = _ents([(3, 21), (0, 20)])
    inputs = {"Tag": _inputs(2)["Tag"]}
    archetype, world, written, after = scatter_ref(handles, [1, 1], [a, b], inputs)
    assert archetype.tolist() == [5, 5] and world.tolist() == [0, 1]
    assert written.tolist() == [1, 1]
    _unchanged([a, b], after, {})


def test_two_tables_in_one_apply():
    a, b = _tables()
    handles = _ents([(0, 20), (5, 12), (3, 21), (0, 20), (1, 6)])
    inputs = _inputs(5)
    archetype, world, written, after = scatter_ref(handles, [1, 1, 1, 1, 0], [a, b], inputs)
    assert archetype.tolist() == [5, 3, 5, 5, 3] and world.tolist() == [1, 1, 0, 1, 1]
    assert written.tolist() == [0, 1, 1, 1, 0]
    assert np.array_equal(after[1].columns["Pos"][0], inputs["Pos"][3])
    assert np.array_equal(after[1].columns["Pos"][1], inputs["Pos"][2])
    assert np.array_equal(after[0].columns["Pos"][4], inputs["Pos"][1])
    assert np.array_equal(after[0].columns["Tag"][4], inputs["Tag"][1])
    _unchanged([a, b], after, {(1, "Pos"): [0, 1], (0, "Pos"): [4], (0, "Tag"): [4]})


def test_it_is_numpy_assignment_one_at_a_time_and_agrees_with_gather_ref():
    """Random handles with many duplicates: the loop of the definition, written
    out here, and gather_ref's archetype and world."""
    a, b = _tables()
    rng = np.random.default_rng(4)
    pool = _ents([(0, 4), (2, 9), (1, 6), (5, 12), (0, 20), (3, 21), NONE, (9, 9), (0, 7)])
    handles = pool[rng.integers(0, len(pool), 200)]
    select = rng.integers(0, 2, 200).astype(np.int32)
    inputs = {"Pos": rng.integers(0, 256, (200, 12)).astype(np.uint8)}
    archetype, world, written, after = scatter_ref(handles, select, [a, b], inputs)
    want = gather_ref(handles, [a, b], [("Pos", 12)])
    assert np.array_equal(archetype, want[0]) and np.array_equal(world, want[1])
    rows = {(0, 4): (0, 0), (2, 9): (0, 1), (1, 6): (0, 2), (5, 12): (0, 4), (0, 20): (1, 0),
            (3, 21): (1, 1)}
    columns = [a.columns["Pos"].copy(), b.columns["Pos"].copy()]
    winner = {}
    for i, h in enumerate(handles.tolist()):
        if select[i] and tuple(h) in rows:
            t, r = rows[tuple(h)]
            columns[t][r] = inputs["Pos"][i]
            winner[tuple(h)] = i
    assert len(winner) == 6
    assert sorted(np.flatnonzero(written).tolist()) == sorted(winner.values())
    assert np.array_equal(after[0].columns["Pos"], columns[0])
    assert np.array_equal(after[1].columns["Pos"], columns[1])
    assert np.array_equal(after[0].columns["Tag"], a.columns["Tag"])


def test_shapes_are_checked():
    a, b = _tables()
    handles = _ents([(2, 9), (0, 4)])
    with pytest.raises(ValueError):
        scatter_ref(handles, [1], [a, b], _inputs(2))
    with pytest.raises(ValueError):
        scatter_ref(handles, [1, 1], [a, b], _inputs(3))
    with pytest.raises(ValueError):
        scatter_ref(handles, [1, 1], [a, b], {"Pos": np.zeros((2, 8), np.uint8)})
