"""CPU-only: madrona_amd/gather_ref.py, the definition of an entity gather, on
hand-made tables."""
import numpy as np
import pytest

from madrona_amd.gather_ref import (Table, gather_ref, read_handles, table_of_dump,
                                    table_of_raw)

NONE = (0xFFFFFFFF, 0xFFFFFFFF)     # Entity::none(): gen 0xFFFFFFFF, id -1


def _ents(pairs):
    return np.array(pairs, dtype=np.uint32).reshape(-1, 2)


def _cells(rows, size, salt):
    return ((np.arange(rows * size).reshape(rows, size) * 7 + salt) % 251).astype(np.uint8)


def _tables():
    """Table 3 (Pos 12 bytes, Tag 1 byte): rows of worlds 0, 0, 1, one row
    destroyed in place (Entity cell still there, WorldID -1), one more of world
    1.  Table 5 (Pos only): two rows of world 1 and 0."""
    a = table_of_raw(3, _ents([(0, 4), (2, 9), (1, 6), (0, 7), (5, 12)]),
                     np.array([0, 0, 1, -1, 1], np.int32),
                     {"Pos": _cells(5, 12, 1), "Tag": _cells(5, 1, 2)})
    b = table_of_raw(5, _ents([(0, 20), (3, 21)]), np.array([1, 0], np.int32),
                     {"Pos": _cells(2, 12, 3)})
    return a, b


COMPONENTS = [("Pos", 12), ("Tag", 1)]


def test_live_stale_none_and_unknown_handles():
    a, b = _tables()
    handles = _ents([(2, 9),        # live, table 3 row 1
                     (1, 9),        # the id is held with another generation
                     NONE,
                     (0, 1000),     # an id nobody has
                     (3, 21),       # live, table 5 row 1
                     (0, 4)])       # live, table 3 row 0
    archetype, world, cells = gather_ref(handles, [a, b], COMPONENTS)
    assert archetype.dtype == np.int32 and world.dtype == np.int32
    assert archetype.tolist() == [3, -1, -1, -1, 5, 3]
    assert world.tolist() == [0, -1, -1, -1, 0, 0]
    assert np.array_equal(cells["Pos"][0], a.columns["Pos"][1])
    assert np.array_equal(cells["Pos"][4], b.columns["Pos"][1])
    assert np.array_equal(cells["Pos"][5], a.columns["Pos"][0])
    assert np.array_equal(cells["Tag"][0], a.columns["Tag"][1])
    for i in (1, 2, 3):
        assert not cells["Pos"][i].any() and not cells["Tag"][i].any()
    assert cells["Pos"].shape == (6, 12) and cells["Tag"].shape == (6, 1)


def test_a_row_destroyed_in_place_names_nothing():
    a, b = _tables()
    archetype, world, cells = gather_ref(_ents([(0, 7)]), [a, b], COMPONENTS)
    assert archetype.tolist() == [-1] and world.tolist() == [-1]
    assert not cells["Pos"].any() and not cells["Tag"].any()
    # ... and the same cell with a live WorldID does
    a.world_ids[3] = 1
    archetype, world, cells = gather_ref(_ents([(0, 7)]), [a, b], COMPONENTS)
    assert archetype.tolist() == [3] and world.tolist() == [1]
    assert np.array_equal(cells["Pos"][0], a.columns["Pos"][3])


def test_a_component_the_table_lacks_gives_zeros():
    a, b = _tables()
    archetype, world, cells = gather_ref(_ents([(0, 20), (5, 12)]), [a, b], COMPONENTS)
    assert archetype.tolist() == [5, 3] and world.tolist() == [1, 1]
    assert np.array_equal(cells["Pos"][0], b.columns["Pos"][0])
    assert not cells["Tag"][0].any()                # table 5 has no Tag
    assert np.array_equal(cells["Tag"][1], a.columns["Tag"][4])


def test_a_negative_id_names_nothing_even_where_a_cell_holds_it():
    """Rows without an entity (temporaries) hold Entity::none() and a live
    WorldID: Entity::none() names none of them, nor does any other negative id."""
    a = table_of_raw(3, _ents([NONE, (0, 4), NONE, (7, 0x80000005)]),
                     np.array([0, 0, 1, 1], np.int32), {"Pos": _cells(4, 12, 6)})
    archetype, world, cells = gather_ref(_ents([NONE, (0, 4), (7, 0x80000005)]), [a],
                                         [("Pos", 12)])
    assert archetype.tolist() == [-1, 3, -1] and world.tolist() == [-1, 0, -1]
    assert not cells["Pos"][0].any() and not cells["Pos"][2].any()


def test_no_components_and_no_tables():
    a, b = _tables()
    archetype, world, cells = gather_ref(_ents([(2, 9), NONE]), [a, b], [])
    assert archetype.tolist() == [3, -1] and cells == {}
    archetype, world, cells = gather_ref(_ents([(2, 9)]), [], COMPONENTS)
    assert archetype.tolist() == [-1] and not cells["Pos"].any()


def test_two_level_source_addressing():
    """Records of 40 bytes, three handles from byte 12 on; what lies around
    them is never read as a handle."""
    record_bytes, first, per, records = 40, 12, 3, 4
    buf = np.full(records * record_bytes + 5, 0xAB, dtype=np.uint8)
    want = []
    for r in range(records):
        for k in range(per):
            gen, ident = 100 * r + k, 7 * r + k + 1
            at = r * record_bytes + first + 8 * k
            buf[at: at + 8] = np.array([gen, ident], "<u4").view(np.uint8)
            want.append((gen, ident))
    got = read_handles(buf, records, record_bytes, first, per)
    assert got.dtype == np.uint32 and got.tolist() == [list(w) for w in want]
    # one handle per 8-byte record: the plain list
    plain = _ents(want)
    assert np.array_equal(read_handles(plain, len(want), 8), plain)
    # a typed buffer is read as its bytes
    as_i32 = np.frombuffer(buf[:160].tobytes(), dtype="<i4")
    assert np.array_equal(read_handles(as_i32, records, record_bytes, first, per), got)
    with pytest.raises(ValueError):
        read_handles(buf, records, record_bytes, 20, per)       # 20 + 24 > 40
    with pytest.raises(ValueError):
        read_handles(buf[:100], records, record_bytes, first, per)


def test_handles_as_bytes_and_as_int32():
    a, b = _tables()
    handles = _ents([(2, 9), NONE, (3, 21)])
    want = gather_ref(handles, [a, b], COMPONENTS)
    for form in (handles.view(np.uint8).reshape(-1, 8), handles.view(np.int32)):
        got = gather_ref(form, [a, b], COMPONENTS)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert all(np.array_equal(got[2][k], want[2][k]) for k in want[2])


def test_table_order_and_per_world_dumps_agree_without_holes():
    """A table sorted by world without holes is its per-world dump; the
    reference backend's dump has no WorldID column."""
    ents = _ents([(0, 4), (2, 9), (1, 6), (5, 12), (0, 30)])
    world_ids = np.array([0, 0, 1, 1, 3], np.int32)      # (world 2 is empty)
    pos, tag = _cells(5, 12, 4), _cells(5, 1, 5)
    counts = np.array([2, 2, 0, 1], np.int32)
    raw = table_of_raw(3, ents.view(np.uint8).reshape(-1, 8),
                       world_ids.view(np.uint8).reshape(-1, 4), {"Pos": pos, "Tag": tag})
    dump = table_of_dump(3, (ents.view(np.uint8).reshape(-1, 8), counts),
                         {"Pos": (pos, counts), "Tag": (tag, counts)})
    assert isinstance(dump, Table) and np.array_equal(dump.world_ids, world_ids)
    handles = _ents([(0, 30), (1, 6), (9, 9), (0, 4), NONE, (5, 12)])
    one = gather_ref(handles, [raw], COMPONENTS)
    two = gather_ref(handles, [dump], COMPONENTS)
    assert one[0].tolist() == [3, 3, -1, 3, -1, 3] and one[1].tolist() == [3, 1, -1, 0, -1, 1]
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    assert all(np.array_equal(one[2][k], two[2][k]) for k in ("Pos", "Tag"))


def test_mismatched_inputs_are_refused():
    with pytest.raises(ValueError):
        table_of_raw(1, _ents([(0, 1)]), np.array([0, 0], np.int32), {})
    with pytest.raises(ValueError):
        table_of_raw(1, _ents([(0, 1)]), np.array([0], np.int32), {"A": _cells(2, 4, 0)})
    a, b = _tables()
    with pytest.raises(ValueError):
        gather_ref(_ents([(2, 9)]), [a], [("Pos", 8)])      # the column has 12-byte cells
