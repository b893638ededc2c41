"""CPU-only: madrona_amd/write_ref.py, the numpy definition of world writes, on
hand-made tables, alone and against view_ref (a write is a view's inverse)."""
import numpy as np
import pytest

from madrona_amd import view_ref, write_ref


def _cells(rows, cell_bytes, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (rows, cell_bytes)).astype(np.uint8)


def _padded(worlds, max_rows, cell_bytes, seed=1):
    # (200 .. 255 against 0 .. 199 below: a written byte is recognisable)
    return np.random.default_rng(seed).integers(200, 256, (worlds, max_rows, cell_bytes)) \
        .astype(np.uint8)


def test_holes_scattered_worlds_and_ids_out_of_range():
    #                 r: 0  1   2  3  4  5   6  7  8  9
    world = np.array([2, 0, -1, 2, 7, 0, -1, 2, 3, 0], np.int32)     # 3 worlds: 7 and 3 are none
    cells = _cells(10, 5) % 200
    padded = _padded(3, 2, 5)
    take = np.array([2, 5, 1], np.int32)
    before = (world.copy(), cells.copy(), padded.copy(), take.copy())
    out, counts = write_ref.write_of_raw(world, cells, padded, take, 3, 2)
    assert counts.dtype == np.int32 and counts.tolist() == [3, 0, 3]
    want = cells.copy()
    want[1], want[5] = padded[0, 0], padded[0, 1]       # world 0: two of its three rows
    want[0] = padded[2, 0]                              # world 2: take 1
    assert np.array_equal(out, want)
    assert out is not cells
    # rows 9 (world 0, third), 3 and 7 (world 2), the holes and the foreign ids: untouched
    for r in (2, 3, 4, 6, 7, 8, 9):
        assert np.array_equal(out[r], cells[r]), r
    for got, was in zip((world, cells, padded, take), before):
        assert np.array_equal(got, was), "an input was modified"
    # the bytes of the WorldID column are accepted as they are dumped
    out8, counts8 = write_ref.write_of_raw(world.view(np.uint8).reshape(-1, 4), cells, padded,
                                           take, 3, 2)
    assert np.array_equal(out8, out) and np.array_equal(counts8, counts)


def test_take_is_clipped_to_zero_to_the_count_and_to_max_rows():
    world = np.array([0, 0, 0, 1, 1, 2, 2, 2, 2, 2], np.int32)
    cells = _cells(10, 3) % 200
    padded = _padded(4, 3, 3)
    #                negative, above count (2), above max_rows (3), world without rows
    take = np.array([-2, 9, 1000, 3], np.int32)
    out, counts = write_ref.write_of_raw(world, cells, padded, take, 4, 3)
    assert counts.tolist() == [3, 2, 5, 0]
    assert np.array_equal(out[0:3], cells[0:3])             # take < 0: nothing
    assert np.array_equal(out[3:5], padded[1, :2])          # the two rows there are
    assert np.array_equal(out[5:8], padded[2])              # max_rows of five
    assert np.array_equal(out[8:10], cells[8:10])           # rows from k on
    zero, _ = write_ref.write_of_raw(world, cells, padded, np.zeros(4, np.int32), 4, 3)
    assert np.array_equal(zero, cells)


def test_empty_table_and_bad_arguments():
    out, counts = write_ref.write_of_raw(np.zeros(0, np.int32), np.zeros((0, 4), np.uint8),
                                         _padded(2, 3, 4), np.array([3, 3], np.int32), 2, 3)
    assert out.shape == (0, 4) and counts.tolist() == [0, 0]
    world, cells = np.zeros(2, np.int32), _cells(2, 4)
    with pytest.raises(ValueError):
        write_ref.write_of_raw(world, cells, _padded(1, 1, 4), [1], 1, 0)
    with pytest.raises(ValueError):
        write_ref.write_of_raw(world, cells[:1], _padded(1, 1, 4), [1], 1, 1)
    with pytest.raises(ValueError):
        write_ref.write_of_raw(world, cells, _padded(1, 2, 4), [1], 1, 1)
    with pytest.raises(ValueError):
        write_ref.write_of_raw(world, cells, _padded(1, 1, 4), [1, 1], 1, 1)


def _random_table(seed, rows=300, worlds=9):
    rng = np.random.default_rng(seed)
    world = rng.integers(-1, worlds + 2, rows).astype(np.int32)     # holes and foreign ids
    return world, _cells(rows, 12, seed + 1)


@pytest.mark.parametrize("max_rows", [1, 7, 64])
def test_writing_a_view_back_changes_nothing(max_rows):
    world, cells = _random_table(3)
    padded, counts = view_ref.view_of_raw(world, cells, 9, max_rows)
    out, write_counts = write_ref.write_of_raw(world, cells, padded,
                                               np.full(9, max_rows, np.int32), 9, max_rows)
    assert np.array_equal(out, cells)
    assert np.array_equal(write_counts, counts)
    if max_rows == 7:
        assert (counts > 7).any(), "no world was truncated"


@pytest.mark.parametrize("max_rows", [1, 7, 64])
def test_a_view_of_a_written_table_shows_the_written_cells(max_rows):
    world, cells = _random_table(5)
    cells %= 200
    padded = _padded(9, max_rows, 12)
    take = np.random.default_rng(6).integers(-2, max_rows + 3, 9).astype(np.int32)
    out, counts = write_ref.write_of_raw(world, cells, padded, take, 9, max_rows)
    seen, seen_counts = view_ref.view_of_raw(world, out, 9, max_rows)
    was, _ = view_ref.view_of_raw(world, cells, 9, max_rows)
    assert np.array_equal(seen_counts, counts)
    k = np.minimum(np.minimum(np.maximum(take, 0), counts), max_rows)
    for w in range(9):
        assert np.array_equal(seen[w, :k[w]], padded[w, :k[w]]), w
        assert np.array_equal(seen[w, k[w]:], was[w, k[w]:]), w
    # exactly the k rows of each world changed, nothing else
    changed = np.flatnonzero((out != cells).any(axis=1))
    assert len(changed) == int(k.sum())
    assert ((world[changed] >= 0) & (world[changed] < 9)).all()
