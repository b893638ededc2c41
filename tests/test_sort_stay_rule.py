"""CPU: the rule behind the compaction chain's stay mode
(madrona_amd/csrc/sort_archetype.hip), on a numpy model of the chain.

The model is the destination formula of the chain's header comment.  A table
is a world-sorted prefix of P rows, some destroyed in place (key 0xFFFFFFFF),
and a tail appended in any world order, some of it destroyed again.  With
s(i) = survivors among prefix rows [0, i), end(w) = the end of world w's old
range and the live tail rows sorted stably by world (j = index in that order):

    prefix row i of world w:  dest = s(i) + #{ tail rows of worlds < w }
    tail row j of world w:    dest = s(end(w)) + j

Stay mode applies when (a) every surviving prefix row has dest == its row and
(b) n_out <= P.  Checked here: the formula is the stable sort; under (a) and
(b) every moved row comes from the tail and goes to a destroyed slot of the
prefix (so the moves need no order and no staging); and (a) without (b) is not
enough, a tail row can then land on a row another move still has to read."""
import numpy as np
import pytest

DEAD = 0xFFFFFFFF


def make_table(rng, worlds, balanced, max_rows=12, extra_tail=None):
    """keys (prefix + tail), per-world prefix counts, P.  balanced: every world
    appends exactly as many live rows as it lost, at the end of its range or
    anywhere in it; otherwise holes and tail rows are independent."""
    counts = rng.integers(0, max_rows + 1, worlds)
    prefix_world = np.repeat(np.arange(worlds), counts)
    keys = prefix_world.astype(np.uint32)
    tail = []
    for w in range(worlds):
        rows = np.nonzero(prefix_world == w)[0]
        lost = int(rng.integers(0, len(rows) + 1)) if rng.random() < 0.4 else 0
        if balanced == "back":
            hit = rows[len(rows) - lost:]
        else:
            hit = rng.choice(rows, lost, replace=False) if lost else rows[:0]
        keys[hit] = DEAD
        if balanced in ("back", "anywhere"):
            new = lost
        else:
            new = int(rng.integers(0, 5)) if rng.random() < 0.4 else 0
        tail += [w] * new
    tail = np.array(tail, dtype=np.uint32)
    rng.shuffle(tail)
    if extra_tail is not None:
        tail = np.concatenate([tail, np.asarray(extra_tail, dtype=np.uint32)])
    # (some tail rows destroyed again: appended and removed in one step)
    dead_again = np.full(int(rng.integers(0, 4)), DEAD, dtype=np.uint32)
    at = rng.integers(0, len(tail) + 1, len(dead_again))
    tail = np.insert(tail, at, dead_again)
    return np.concatenate([keys, tail]), counts, len(keys)


def chain_destinations(keys, counts, prefix):
    """dest of every row by the chain's formula (-1: dropped), and n_out."""
    n = len(keys)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    live_prefix = keys[:prefix] != DEAD
    s = np.concatenate([[0], np.cumsum(live_prefix)])          # s(i), i in [0, P]
    tail_keys = keys[prefix:]
    tail_live = np.nonzero(tail_keys != DEAD)[0]
    order = tail_live[np.argsort(tail_keys[tail_live], kind="stable")]
    sorted_worlds = tail_keys[order].astype(np.int64)

    dest = np.full(n, -1, dtype=np.int64)
    prefix_world = np.repeat(np.arange(len(counts)), counts)
    tail_before_world = np.searchsorted(sorted_worlds, prefix_world, side="left")
    rows = np.nonzero(live_prefix)[0]
    dest[rows] = s[rows] + tail_before_world[rows]
    end = offsets[1:]
    dest[prefix + order] = s[end[sorted_worlds]] + np.arange(len(order))
    return dest, int(live_prefix.sum()) + len(order)


def stable_sort(keys):
    perm = np.argsort(keys, kind="stable")
    return perm[keys[perm] != DEAD]


def rule(keys, prefix, dest, n_out):
    live_prefix = np.nonzero(keys[:prefix] != DEAD)[0]
    a = bool((dest[live_prefix] == live_prefix).all())
    b = n_out <= prefix
    return a, b


@pytest.mark.parametrize("balanced", ["back", "anywhere", "no"])
def test_formula_is_the_stable_sort_and_stay_moves_are_independent(balanced):
    rng = np.random.default_rng({"back": 1, "anywhere": 2, "no": 3}[balanced])
    stayed = 0
    for trial in range(300):
        worlds = int(rng.integers(1, 40))
        keys, counts, prefix = make_table(rng, worlds, balanced)
        dest, n_out = chain_destinations(keys, counts, prefix)

        # the formula is the stable sort by world, destroyed rows dropped
        perm = stable_sort(keys)
        assert n_out == len(perm)
        placed = np.full(n_out, -1, dtype=np.int64)
        rows = np.nonzero(dest >= 0)[0]
        placed[dest[rows]] = rows
        assert np.array_equal(placed, perm), (balanced, trial)

        a, b = rule(keys, prefix, dest, n_out)
        if not (a and b):
            continue
        stayed += 1
        moved = np.nonzero((dest >= 0) & (dest != np.arange(len(keys))))[0]
        assert (moved >= prefix).all(), "a moved row that is not a tail row"
        assert (dest[moved] < prefix).all()
        assert (keys[dest[moved]] == DEAD).all(), "a destination that is no destroyed slot"
        assert len(set(dest[moved])) == len(moved)
        assert not set(dest[moved]) & set(moved), "a destination is a source"
        # patching the moved rows in place gives the sorted table
        patched = keys.copy()
        patched[dest[moved]] = keys[moved]
        assert np.array_equal(patched[:n_out], keys[perm]), (balanced, trial)
    if balanced == "back":
        # rows lost at the back of a world's range and replaced: every trial
        assert stayed == 300
    elif balanced == "anywhere":
        assert stayed > 0
    else:
        assert stayed < 300


def test_a_without_b_can_land_on_a_source():
    rng = np.random.default_rng(7)
    found = 0
    for trial in range(100):
        worlds = int(rng.integers(3, 40))
        # balanced, except that the last world grows by two
        keys, counts, prefix = make_table(rng, worlds, "back",
                                          extra_tail=[worlds - 1, worlds - 1])
        dest, n_out = chain_destinations(keys, counts, prefix)
        assert np.array_equal(
            np.argsort(np.where(dest >= 0, dest, len(keys)), kind="stable")[:n_out],
            stable_sort(keys))
        a, b = rule(keys, prefix, dest, n_out)
        assert a and not b, trial
        moved = np.nonzero((dest >= 0) & (dest != np.arange(len(keys))))[0]
        sources = set(moved)
        on_source = [r for r in moved if dest[r] in sources]
        if on_source:
            assert all(r >= prefix and dest[r] >= prefix for r in on_source)
            found += 1
    assert found > 0, "no input where a tail row lands on another tail row's place"
