"""CPU-only: madrona_amd/view_ref.py, the numpy definition of a world view (the
yardstick of tests/test_world_view_gpu.py), on hand-written tables."""
import numpy as np
import pytest

from madrona_amd import view_ref


def _cells(values, width):
    """row i holds `width` bytes: values[i], values[i] + 1, ..."""
    v = np.asarray(values, dtype=np.int64)[:, None] + np.arange(width)[None, :]
    return (v % 256).astype(np.uint8)


def test_sorted_table_with_an_empty_world():
    world = np.array([0, 0, 2, 2, 2, 3], np.int32)
    cells = _cells([10, 20, 30, 40, 50, 60], 12)
    padded, counts = view_ref.view_of_raw(world, cells, 4, 3)
    assert padded.dtype == np.uint8 and padded.shape == (4, 3, 12)
    assert counts.dtype == np.int32 and counts.tolist() == [2, 0, 3, 1]
    assert np.array_equal(padded[0, :2], cells[:2]) and not padded[0, 2].any()
    assert not padded[1].any()
    assert np.array_equal(padded[2], cells[2:5])
    assert np.array_equal(padded[3, 0], cells[5]) and not padded[3, 1:].any()


def test_holes_belong_to_no_world():
    world = np.array([0, -1, 0, 1, -1, -1, 1], np.int32)
    cells = _cells([1, 2, 3, 4, 5, 6, 7], 1)
    padded, counts = view_ref.view_of_raw(world, cells, 2, 4)
    assert counts.tolist() == [2, 2]
    assert padded[0, :, 0].tolist() == [1, 3, 0, 0]
    assert padded[1, :, 0].tolist() == [4, 7, 0, 0]
    # a table of nothing but holes, and ids past the last world
    padded, counts = view_ref.view_of_raw(np.array([-1, -1, 5], np.int32), _cells([1, 2, 3], 1),
                                          2, 2)
    assert counts.tolist() == [0, 0] and not padded.any()


def test_unsorted_tail_keeps_table_order():
    # a sorted prefix (worlds 0, 1, 2), then rows appended in any order
    world = np.array([0, 1, 1, 2, 2, 0, 1, 0], np.int32)
    cells = _cells([10, 20, 21, 30, 31, 11, 22, 12], 12)
    padded, counts = view_ref.view_of_raw(world, cells, 3, 4)
    assert counts.tolist() == [3, 3, 2]
    assert padded[0, :, 0].tolist() == [10, 11, 12, 0]
    assert padded[1, :, 0].tolist() == [20, 21, 22, 0]
    assert padded[2, :, 0].tolist() == [30, 31, 0, 0]
    assert np.array_equal(padded[0, 2], cells[7])
    # fully descending ids
    padded, counts = view_ref.view_of_raw(np.array([2, 1, 1, 0], np.int32),
                                          _cells([5, 6, 7, 8], 1), 3, 2)
    assert padded[:, :, 0].tolist() == [[8, 0], [6, 7], [5, 0]]


def test_truncation_reports_the_full_count():
    world = np.array([1, 0, 1, 1, -1, 1, 0, 1], np.int32)
    cells = _cells([1, 2, 3, 4, 5, 6, 7, 8], 12)
    padded, counts = view_ref.view_of_raw(world, cells, 2, 3)
    assert counts.tolist() == [2, 5]            # not clipped to max_rows
    # the first three of world 1 in table order; the later ones are dropped
    assert padded[1, :, 0].tolist() == [1, 3, 4]
    assert np.array_equal(padded[1], cells[[0, 2, 3]])
    assert padded[0, :, 0].tolist() == [2, 7, 0]
    one, counts = view_ref.view_of_raw(world, cells, 2, 1)
    assert one.shape == (2, 1, 12) and one[:, 0, 0].tolist() == [2, 1]
    assert counts.tolist() == [2, 5]


def test_no_rows_at_all():
    padded, counts = view_ref.view_of_raw(np.zeros(0, np.int32), np.zeros((0, 12), np.uint8), 3, 2)
    assert padded.shape == (3, 2, 12) and not padded.any() and counts.tolist() == [0, 0, 0]


def test_world_ids_as_bytes_and_bad_arguments():
    world = np.array([1, -1, 0], np.int32)
    cells = _cells([9, 8, 7], 1)
    a = view_ref.view_of_raw(world, cells, 2, 2)
    b = view_ref.view_of_raw(world.view(np.uint8).reshape(3, 4), cells, 2, 2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        view_ref.view_of_raw(world, cells, 2, 0)
    with pytest.raises(ValueError):
        view_ref.view_of_raw(world, cells[:2], 2, 2)


def test_view_of_a_per_world_dump():
    rows = _cells([1, 2, 3, 4], 12)
    padded, counts = view_ref.view_of_dump(rows, np.array([1, 0, 3], np.int32), 3, 2)
    assert counts.tolist() == [1, 0, 3]
    assert padded[:, :, 0].tolist() == [[1, 0], [0, 0], [2, 3]]
