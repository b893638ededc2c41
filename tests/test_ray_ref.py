"""CPU-only: madrona_amd/ray_ref.py, the definition of a ray query, against
hand-worked cases.  The tracer is the module's own brute-force slab tracer over
axis-aligned boxes; the device tests inject the simulators' ray systems instead."""
import numpy as np
import pytest

from madrona_amd import ray_ref
from madrona_amd.ray_ref import (BAD_RAY, BAD_WORLD, HIT, MISS, SKIPPED, as_source, box_tracer,
                                 ray_ref as query)

INF = np.float32(np.inf)
NONE = [0xFFFFFFFF, 0xFFFFFFFF]

# world 0: a unit cube centred at (5, 0, 0) and a slab behind it; world 1: empty;
# world 2: a cube above the origin
WORLDS = [
    [((4.5, -0.5, -0.5), (5.5, 0.5, 0.5), (3, 7)), ((8, -4, -4), (9, 4, 4), (0, 11))],
    [],
    [((-1, -1, 2), (1, 1, 4), (1, 2))],
]
TRACE = box_tracer(WORLDS)


def _run(fans, rays, directions, origins, worlds=None, t_max=None, **kw):
    n = fans * rays
    return query(TRACE, len(WORLDS), fans, rays,
                 directions=np.asarray(directions, np.float32).reshape(n, 3),
                 t_max=np.full(n, INF, np.float32) if t_max is None else t_max,
                 origin=as_source(np.asarray(origins, np.float32).reshape(fans, 3), np.float32),
                 world=None if worlds is None else as_source(np.asarray(worlds), np.int32), **kw)


def test_hand_worked_hits_and_misses():
    # one fan of four rays from the origin of world 0
    hit_t, hit, normal, status = _run(
        1, 4, [[1, 0, 0], [2, 0, 0], [0, 1, 0], [1, 0.25, 0]], [[0, 0, 0]], worlds=[0])
    assert status.tolist() == [HIT, HIT, MISS, HIT]
    # the cube's near face at x = 4.5; a direction of length 2 halves t
    assert hit_t.tolist() == [4.5, 2.25, 0.0, 8.0]
    assert hit.tolist() == [[3, 7], [3, 7], NONE, [0, 11]]
    assert normal.tolist() == [[-1, 0, 0], [-1, 0, 0], [0, 0, 0], [-1, 0, 0]]
    assert hit_t.dtype == np.float32 and hit.dtype == np.uint32
    assert normal.dtype == np.float32 and status.dtype == np.int32


def test_t_max_cuts_a_ray_and_the_closest_box_wins():
    t_max = np.array([4.0, 4.5, 1e9], np.float32)
    hit_t, hit, _, status = _run(1, 3, [[1, 0, 0]] * 3, [[0, 0, 0]], worlds=[0], t_max=t_max)
    assert status.tolist() == [MISS, HIT, HIT] and hit_t.tolist() == [0.0, 4.5, 4.5]
    # from behind the cube only the slab is ahead; from inside the cube it is
    # transparent
    hit_t, hit, _, status = _run(2, 1, [[1, 0, 0]] * 2, [[6, 0, 0], [5, 0, 0]], worlds=[0, 0])
    assert hit_t.tolist() == [2.0, 3.0] and hit.tolist() == [[0, 11], [0, 11]]


def test_fans_share_world_and_origin_and_worlds_differ():
    directions = [[1, 0, 0], [0, 0, 1]] * 3
    hit_t, hit, normal, status = _run(3, 2, directions, [[0, 0, 0]] * 3, worlds=[0, 1, 2])
    assert status.tolist() == [HIT, MISS, MISS, MISS, MISS, HIT]
    assert hit_t.tolist() == [4.5, 0, 0, 0, 0, 2.0]
    assert hit[5].tolist() == [1, 2] and normal[5].tolist() == [0, 0, -1]


def test_every_status():
    nan = np.float32(np.nan)
    worlds = [0, -1, 3, -2 ** 31, 0, 0, 0, 0]
    origins = [[0, 0, 0]] * 4 + [[nan, 0, 0], [0, INF, 0], [0, 0, 0], [0, 0, 0]]
    directions = np.tile(np.float32([1, 0, 0]), (8, 2, 1))
    directions[6, 0] = [0, 0, 0]
    directions[6, 1] = [1, -INF, 0]
    directions[7, 0] = [nan, 1, 0]
    t_max = np.full(16, INF, np.float32)
    t_max[15] = nan
    hit_t, hit, normal, status = _run(8, 2, directions, origins, worlds=worlds, t_max=t_max)
    assert status.reshape(8, 2).tolist() == [
        [HIT, HIT], [BAD_WORLD] * 2, [BAD_WORLD] * 2, [BAD_WORLD] * 2, [BAD_RAY] * 2,
        [BAD_RAY] * 2, [BAD_RAY] * 2, [BAD_RAY] * 2]
    # anything but a hit: 0, none, zero
    rest = status != HIT
    assert not hit_t[rest].any() and not normal[rest].any()
    assert (hit[rest] == 0xFFFFFFFF).all()
    # -inf and +inf are t_max values like any other
    t_max = np.array([-INF, INF], np.float32)
    _, _, _, status = _run(1, 2, [[1, 0, 0]] * 2, [[0, 0, 0]], worlds=[0], t_max=t_max)
    assert status.tolist() == [MISS, HIT]


def test_a_bad_ray_leaves_its_neighbours_alone():
    directions = [[1, 0, 0], [0, 0, 0], [1, 0, 0]]
    hit_t, _, _, status = _run(1, 3, directions, [[0, 0, 0]], worlds=[0])
    assert status.tolist() == [HIT, BAD_RAY, HIT] and hit_t.tolist() == [4.5, 0, 4.5]


def test_strides_and_offsets():
    """Worlds inside 8-byte records at byte 4, origins inside 20-byte records
    at byte 8; the bytes around them are poison."""
    F = 3
    wbuf = np.full((F, 2), 0x7FFFFFFF, np.int32)
    wbuf[:, 1] = [2, 0, 1]
    obuf = np.full((F, 5), np.nan, np.float32)
    obuf[:, 2:5] = [[0, 0, 0], [0, 0, 0], [0, 0, 0]]
    out = query(TRACE, 3, F, 1, directions=np.float32([[0, 0, 1], [1, 0, 0], [1, 0, 0]]),
                t_max=np.full(F, INF, np.float32), origin=(obuf.view(np.uint8), 20, 8),
                world=(wbuf.view(np.uint8), 8, 4))
    assert out[3].tolist() == [HIT, HIT, MISS] and out[0].tolist() == [2.0, 4.5, 0.0]
    for bad in ((obuf.view(np.uint8), 20, 12), (obuf.view(np.uint8), 18, 0),
                (obuf.view(np.uint8), 20, 2)):
        with pytest.raises(ValueError):
            query(TRACE, 3, F, 1, directions=np.ones((F, 3), np.float32),
                  t_max=np.full(F, INF, np.float32), origin=bad, world=(wbuf.view(np.uint8), 8, 4))


@pytest.mark.parametrize("max_rows", [1, 3])
def test_fans_per_world_with_counts_0_1_and_max_rows(max_rows):
    """The shape of a world view's slab: world = f // max_rows, and the fans
    past a world's count are skipped -- their origins (padding) are not read."""
    W = 3
    counts = np.array([max_rows, 0, 1], np.int32)
    origins = np.full((W, max_rows, 3), np.nan, np.float32)
    for w in range(W):
        origins[w, :counts[w]] = 0
    F = W * max_rows
    directions = np.tile(np.float32([[1, 0, 0], [0, 0, 1]]), (F, 1))
    hit_t, hit, _, status = query(
        TRACE, W, F, 2, directions=directions, t_max=np.full(2 * F, INF, np.float32),
        origin=as_source(origins.reshape(F, 3), np.float32), fans_per_world=max_rows,
        count=as_source(counts, np.int32))
    status = status.reshape(W, max_rows, 2)
    assert (status[0] == [HIT, MISS]).all()
    assert (status[1] == SKIPPED).all()
    assert (status[2, 0] == [MISS, HIT]).all() and (status[2, 1:] == SKIPPED).all()
    assert not hit_t.reshape(W, max_rows, 2)[1].any()
    # without counts the padding is cast like any other fan: NaN origins
    _, _, _, status = query(
        TRACE, W, F, 2, directions=directions, t_max=np.full(2 * F, INF, np.float32),
        origin=as_source(origins.reshape(F, 3), np.float32), fans_per_world=max_rows)
    assert (status.reshape(W, max_rows, 2)[1] == BAD_RAY).all()
    # a world past the last is a bad world even by the rule
    _, _, _, status = query(
        TRACE, W - 1, F, 2, directions=directions, t_max=np.full(2 * F, INF, np.float32),
        origin=as_source(origins.reshape(F, 3), np.float32), fans_per_world=max_rows,
        count=as_source(counts, np.int32))
    assert (status.reshape(W, max_rows, 2)[2] == BAD_WORLD).all()


def test_what_the_definition_refuses():
    ok = dict(directions=np.ones((2, 3), np.float32), t_max=np.ones(2, np.float32),
              origin=as_source(np.zeros((2, 3)), np.float32))
    with pytest.raises(ValueError):
        query(TRACE, 3, 2, 1, **ok)                                     # no world at all
    with pytest.raises(ValueError):
        query(TRACE, 3, 2, 1, world=as_source(np.zeros(2), np.int32),
              count=as_source(np.zeros(3), np.int32), **ok)             # counts without the rule
    with pytest.raises(ValueError):
        query(TRACE, 3, 0, 1, fans_per_world=1, **ok)


def test_the_tracer_is_injected():
    calls = []

    def trace(w, o, d, t_max):
        calls.append((w, tuple(o), tuple(d), float(t_max)))
        return (np.float32(1.5), (0, 1, 0), (9, -5)) if len(calls) == 2 else None

    hit_t, hit, normal, status = query(
        trace, 4, 1, 2, directions=np.float32([[1, 2, 3], [4, 5, 6]]),
        t_max=np.float32([7, 8]), origin=as_source(np.float32([[9, 10, 11]]), np.float32),
        world=as_source(np.array([3]), np.int32))
    assert calls == [(3, (9, 10, 11), (1, 2, 3), 7.0), (3, (9, 10, 11), (4, 5, 6), 8.0)]
    assert status.tolist() == [MISS, HIT] and hit_t.tolist() == [0, 1.5]
    assert hit[1].tolist() == [9, 0xFFFFFFFB] and normal[1].tolist() == [0, 1, 0]


def test_module_constants():
    assert (ray_ref.HIT, ray_ref.MISS, ray_ref.SKIPPED, ray_ref.BAD_WORLD, ray_ref.BAD_RAY) == \
        (1, 0, -1, -2, -3)
