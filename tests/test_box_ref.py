"""CPU-only: the numpy definition of box queries (madrona_amd/box_ref.py), worked
by hand on a made-up world: report order, K truncation, every status, the order
of the checks and an unbuilt tree."""
import numpy as np
import pytest

from madrona_amd import box_ref
from madrona_amd.box_ref import BAD_BOX, BAD_WORLD, OK, SKIPPED, as_source, box_ref as ref

NONE = 0xFFFFFFFF
# world 0, in traversal order: four unit cubes along x at 0, 2, 4, 6 (ids 13, 10,
# 12, 11 -- the order is the tree's, not the ids'); world 1: one cube; world 2:
# never built
CUBES = [
    [((x - 0.5, -0.5, -0.5), (x + 0.5, 0.5, 0.5), (7, i))
     for x, i in ((0, 13), (2, 10), (4, 12), (6, 11))],
    [((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (3, 20))],
    None,
]
ENUM = box_ref.cube_enumerator(CUBES)


def _run(worlds, centres, lo, hi, K=3, G=None, **kwargs):
    F = len(centres)
    G = len(lo) // F if G is None else G
    sources = dict(centre=as_source(np.float32(centres), np.float32))
    if worlds is not None:
        sources["world"] = as_source(np.int32(worlds), np.int32)
    return ref(ENUM, len(CUBES), F, G, K, lo=lo, hi=hi, **sources, **kwargs)


def _ids(hits, b):
    return [int(i) for g, i in hits[b] if g != NONE]


def test_order_is_the_enumerations_and_k_truncates_the_list_not_the_count():
    lo = [[-1, -1, -1], [1.6, -1, -1], [-1, -1, -1]]
    hi = [[7, 1, 1], [4.4, 1, 1], [1.5, 1, 1]]
    status, count, hits = _run([0], [[0, 0, 0]], lo, hi)
    assert status.tolist() == [OK, OK, OK]
    assert count.tolist() == [4, 2, 1]                  # (not capped by K = 3)
    assert _ids(hits, 0) == [13, 10, 12]                # report order, the first K
    assert _ids(hits, 1) == [10, 12]
    assert _ids(hits, 2) == [13]
    assert hits.shape == (3, 3, 2) and hits.dtype == np.uint32
    assert (hits[1, 2] == NONE).all() and (hits[2, 1:] == NONE).all()
    assert hits[0, 0].tolist() == [7, 13]               # (gen, id)
    # K = 1 gives the prefix and the same count
    _, count1, hits1 = _run([0], [[0, 0, 0]], lo, hi, K=1)
    assert count1.tolist() == [4, 2, 1] and np.array_equal(hits1, hits[:, :1])


def test_boxes_that_only_touch_do_not_overlap_and_the_centre_moves_the_box():
    status, count, hits = _run([0, 0], [[0, 0, 0], [2, 0, 0]],
                               [[0.5, -1, -1], [-0.5, -0.25, -0.25]],
                               [[1.5, 1, 1], [0.5, 0.25, 0.25]])
    assert status.tolist() == [OK, OK]
    assert count.tolist() == [0, 1]         # [0.5, 1.5] touches both neighbours; 2 + [-0.5, 0.5]
    assert _ids(hits, 1) == [10]
    assert (hits[0] == NONE).all()


def test_every_status_in_the_order_of_the_checks():
    nan, inf = np.nan, np.inf
    worlds = [-1, 3, 0, 0, 0, 0, 1, 2**31 - 1]
    centres = [[nan] * 3, [0] * 3, [0, inf, 0], [0] * 3, [3e38, 0, 0], [0] * 3, [0] * 3, [0] * 3]
    lo = [[-1] * 3] * 8
    hi = [[1] * 3] * 8
    lo[3] = [-1, nan, -1]               # a box's own field
    hi[4] = [3e38, 1, 1]                # the sum overflows
    lo[5], hi[5] = [1, -1, -1], [0.5, 1, 1]     # inverted on x
    status, count, hits = _run(worlds, centres, lo, hi)
    assert status.tolist() == [BAD_WORLD, BAD_WORLD, BAD_BOX, BAD_BOX, BAD_BOX, BAD_BOX, OK,
                               BAD_WORLD]
    assert count.tolist() == [0, 0, 0, 0, 0, 0, 1, 0]
    assert _ids(hits, 6) == [20] and (np.delete(hits, 6, axis=0) == NONE).all()


def test_counts_skip_before_the_centre_is_looked_at():
    count = as_source(np.int32([1, 2, 0]), np.int32)
    centres = [[0] * 3, [np.nan] * 3, [0] * 3, [np.nan] * 3, [np.nan] * 3, [np.nan] * 3]
    status, counts, hits = _run(None, centres, [[-1] * 3] * 6, [[1] * 3] * 6,
                                bundles_per_world=2, count=count)
    # world 0: row 1 is skipped (its NaN centre unread); world 1: row 1 exists and
    # is bad; world 2: both rows skipped
    assert status.tolist() == [OK, SKIPPED, OK, BAD_BOX, SKIPPED, SKIPPED]
    assert counts.tolist() == [1, 0, 1, 0, 0, 0]
    assert _ids(hits, 0) == [13] and _ids(hits, 2) == [20]


def test_a_bad_world_by_the_rule_comes_before_its_count():
    """More bundles than worlds x bundles_per_world: the bundles past the last
    world are BAD_WORLD, and the count source -- exactly one record per world --
    is not indexed by a world that does not exist (int() of the empty read
    would raise)."""
    count = as_source(np.int32([2, 1, 2]), np.int32)
    centres = [[0] * 3] * 6 + [[np.nan] * 3] * 3
    status, counts, hits = _run(None, centres, [[-1] * 3] * 9, [[1] * 3] * 9,
                                bundles_per_world=2, count=count)
    assert status.tolist() == [OK, OK, OK, SKIPPED, OK, OK, BAD_WORLD, BAD_WORLD, BAD_WORLD]
    assert counts.tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0]      # (world 2 was never built)
    assert (hits[3:] == NONE).all()
    assert box_ref.read_source(count, 3, np.int32, 1).size == 0    # (nothing there to read)


def test_an_unbuilt_tree_gives_ok_and_nothing():
    status, count, hits = _run([2, 2], [[0] * 3] * 2, [[-9] * 3] * 2, [[9] * 3] * 2)
    assert status.tolist() == [OK, OK] and not count.any() and (hits == NONE).all()


def test_bundles_share_a_centre_and_sources_have_strides():
    # centre in words 1..3 of records of 5 floats, world in word 2 of 3
    crec = np.full((2, 5), np.nan, np.float32)
    crec[:, 1:4] = [[4, 0, 0], [0, 0, 0]]
    wrec = np.full((2, 3), 99, np.int32)
    wrec[:, 2] = [0, 1]
    lo = [[-0.6, -1, -1], [-2.6, -1, -1], [-0.6, -1, -1], [-2.6, -1, -1]]
    hi = [[0.6, 1, 1], [2.6, 1, 1], [0.6, 1, 1], [2.6, 1, 1]]
    status, count, hits = ref(ENUM, 3, 2, 2, 4, lo=lo, hi=hi,
                              centre=(crec.view(np.uint8).ravel(), 20, 4),
                              world=(wrec.view(np.uint8).ravel(), 12, 8))
    assert not status.any() and count.tolist() == [1, 3, 1, 1]
    assert _ids(hits, 1) == [10, 12, 11] and _ids(hits, 0) == [12]


def test_what_the_definition_refuses():
    with pytest.raises(ValueError):
        _run([0], [[0] * 3], [[0] * 3], [[0] * 3], K=0)
    with pytest.raises(ValueError):
        ref(ENUM, 3, 1, 1, 1, lo=[[0] * 3], hi=[[0] * 3], centre=as_source(np.zeros((1, 3)),
                                                                            np.float32))
    with pytest.raises(ValueError):
        _run([0], [[0] * 3], [[0] * 3], [[0] * 3], count=as_source(np.int32([1]), np.int32))
    with pytest.raises(ValueError):
        ref(ENUM, 3, 2**16, 2**8, 2**7, lo=[], hi=[], centre=None, bundles_per_world=1)
