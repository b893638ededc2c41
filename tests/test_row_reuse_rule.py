"""Row reuse of the ordered create / destroy (madrona/state.inl, OrderedRows::Reuse)
and the sort chain's "every hole was refilled" test (csrc/sort_archetype.hip,
tableRefilled), as a numpy model, against the definition of a world sort: tag the
destroyed rows, append the new ones, sort stably by world.

The model follows the device code step for step:
  destroy   per archetype of the call, the freed rows are remembered when they
            are exactly the last k rows of the world's range [a, a + c) of the
            sorted prefix (a + c <= sortedRows, all of them in [a + c - k, a + c)),
            at most four records per invocation, one per archetype; otherwise the
            table's plainDestroys is set
  create    rows of an archetype with a record take next_row + rank while the
            record lasts, the others append
  sort      skipped when needsSort, sortedRows > 0, numRows == sortedRows,
            plainDestroys == 0 and orderedFreed == orderedRefilled
The plan is sims/sort_stress's (Config::reusePlan): whole range / proper suffix
with as many, fewer, more creates, a subset that is no suffix, two and five
archetypes in one call, worlds without rows."""
import numpy as np
import pytest

TABLES = 5
MAX_ROWS = 8
MAX_RECORDS = 4


class Table:
    def __init__(self):
        self.world = np.zeros(0, np.int64)      # -1: destroyed
        self.uid = np.zeros(0, np.int64)
        self.sorted_rows = 0
        self.needs_sort = False
        self.offsets = None
        self.counts = None
        self.freed = self.refilled = self.plain = 0
        self.reused_total = 0       # never reset

    def copy(self):
        t = Table()
        t.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v)
                           for k, v in self.__dict__.items()})
        return t

    def append(self, world, uid):
        self.world = np.append(self.world, world)
        self.uid = np.append(self.uid, uid)
        self.needs_sort = True
        return len(self.world) - 1

    def world_sort(self, worlds):
        order = np.argsort(np.where(self.world < 0, worlds, self.world), kind="stable")
        order = order[self.world[order] >= 0]
        self.world, self.uid = self.world[order], self.uid[order]
        self.sorted_rows = len(self.world)
        self.needs_sort = False
        self.counts = np.bincount(self.world, minlength=worlds)
        self.offsets = np.cumsum(self.counts) - self.counts
        self.freed = self.refilled = self.plain = 0

    def refilled_in_place(self):
        return (self.needs_sort and self.sorted_rows > 0 and
                len(self.world) == self.sorted_rows and self.plain == 0 and
                self.freed == self.refilled)


def _suffix(n, k):
    return list(range(n - k, n))


def _plan(kind, held):
    """(rows to destroy per table, as positions in the world's list; creates)"""
    n0 = held[0]
    half = (n0 + 1) // 2
    destroy = [[] for _ in range(TABLES)]
    create = [0] * TABLES
    if kind == 0:
        destroy[0], create[0] = _suffix(n0, n0), n0
    elif kind == 1:
        destroy[0], create[0] = _suffix(n0, half), half
    elif kind == 2:
        destroy[0], create[0] = _suffix(n0, half), max(half - 1, 0)
    elif kind == 3:
        destroy[0], create[0] = _suffix(n0, half), half + 2
    elif kind == 4:
        destroy[0], create[0] = ([0] if n0 >= 2 else []), 1
    elif kind == 5:
        destroy[0], create[0] = _suffix(n0, half), half
        destroy[1], create[1] = _suffix(held[1], held[1]), held[1]
    elif kind == 6:
        for a in range(TABLES):
            destroy[a], create[a] = _suffix(held[a], min(held[a], 1)), 1
    else:
        destroy[0], create[0] = _suffix(n0, n0), 0
    for a in range(TABLES):
        create[a] = min(create[a], MAX_ROWS - (held[a] - len(destroy[a])))
    return destroy, create


class Model:
    """One simulator: `worlds` worlds, TABLES tables, the rows each world holds
    (row indices in table order), stepped with and without reuse."""

    def __init__(self, worlds, rng, cold):
        self.worlds = worlds
        self.rng = rng
        self.next_uid = 0
        self.plain = [Table() for _ in range(TABLES)]
        for w in range(worlds):
            for a in range(TABLES):
                for _ in range(int(rng.integers(0, 6))):
                    self.plain[a].append(w, self._uid())
        if not cold:
            for t in self.plain:
                t.world_sort(worlds)
        self.reuse = [t.copy() for t in self.plain]

    def _uid(self):
        self.next_uid += 1
        return self.next_uid

    @staticmethod
    def _rows_of(table, w):
        return np.nonzero(table.world == w)[0]

    def step(self, kinds):
        """One launch of the reset system and the sort node behind it.  Returns
        per table whether the reuse side skipped its sort."""
        order = self.rng.permutation(self.worlds)
        for w in order:
            held = [len(self._rows_of(t, w)) for t in self.plain]
            assert held == [len(self._rows_of(t, w)) for t in self.reuse]
            destroy, create = _plan(kinds[w], held)
            uids = [[self._uid() for _ in range(create[a])] for a in range(TABLES)]

            # the definition: tag, append
            for a, t in enumerate(self.plain):
                rows = self._rows_of(t, w)
                if destroy[a]:
                    t.world[rows[destroy[a]]] = -1
                    t.needs_sort = True
                    t.plain = 1
                for uid in uids[a]:
                    t.append(w, uid)

            # the rule
            records = {}
            for a, t in enumerate(self.reuse):      # (archetypes in lane order)
                if not destroy[a]:
                    continue
                rows = self._rows_of(t, w)
                freed = rows[destroy[a]]
                t.world[freed] = -1
                t.needs_sort = True
                k = len(freed)
                ok = t.sorted_rows > 0
                if ok:
                    lo, c = int(t.offsets[w]), int(t.counts[w])
                    ok = (k <= c and lo + c <= t.sorted_rows and
                          bool(((freed >= lo + c - k) & (freed < lo + c)).all()))
                if ok and len(records) < MAX_RECORDS and a not in records:
                    records[a] = [lo + c - k, k]
                    t.freed += k
                else:
                    t.plain = 1
            for a, t in enumerate(self.reuse):
                for uid in uids[a]:
                    rec = records.get(a)
                    if rec is not None and rec[1] > 0:
                        assert t.world[rec[0]] == -1
                        t.world[rec[0]], t.uid[rec[0]] = w, uid
                        rec[0] += 1
                        rec[1] -= 1
                        t.refilled += 1
                        t.reused_total += 1
                    else:
                        t.append(w, uid)

        skipped = []
        for a in range(TABLES):
            ref, t = self.plain[a], self.reuse[a]
            dirty = ref.needs_sort
            if dirty:
                ref.world_sort(self.worlds)
            if t.refilled_in_place():
                # the chain does nothing: the table must already be the sorted one
                skipped.append(True)
                t.needs_sort = False
            else:
                skipped.append(False)
                if t.needs_sort:
                    t.world_sort(self.worlds)
            assert t.needs_sort is False and dirty in (True, False)
            assert np.array_equal(t.world, ref.world), (a, "worlds")
            assert np.array_equal(t.uid, ref.uid), (a, "rows")
            if ref.offsets is not None:
                assert np.array_equal(t.offsets, ref.offsets), (a, "offsets")
                assert np.array_equal(t.counts, ref.counts), (a, "counts")
                assert t.sorted_rows == ref.sorted_rows
        return skipped


@pytest.mark.parametrize("seed", range(8))
def test_reuse_equals_tag_append_stable_sort(seed):
    """A few thousand world-steps of the plan per seed, cycled and random."""
    rng = np.random.default_rng(seed)
    skips = 0
    for case in range(12):
        worlds = int(rng.choice([1, 2, 3, 7, 20]))
        m = Model(worlds, rng, cold=case % 4 == 0)
        for step in range(16):
            if case % 2 == 0:
                kinds = (np.arange(worlds) + step) % 8      # the simulator's cycle
            else:
                kinds = rng.integers(0, 8, worlds)
            skips += sum(m.step(kinds))
    assert skips > 0


def test_balanced_resets_skip_and_anything_else_does_not():
    rng = np.random.default_rng(0)
    m = Model(6, rng, cold=False)
    # whole range and proper suffix with as many creates: table 0 stays in order
    skipped = m.step(np.array([0, 1, 0, 1, 0, 1]))
    assert skipped[0] is True
    # one world creates fewer than it freed: a hole is left, the chain runs
    if len(Model._rows_of(m.plain[0], 2)) >= 3:
        assert m.step(np.array([0, 1, 2, 1, 0, 1]))[0] is False
    # one world appends past what it freed
    assert m.step(np.array([0, 1, 0, 3, 0, 1]))[0] is False
    # a destroy that is no suffix, next to balanced resets
    rows = [len(Model._rows_of(m.plain[0], w)) for w in range(6)]
    if rows[4] >= 2:
        assert m.step(np.array([0, 1, 0, 1, 4, 1]))[0] is False


def test_cold_table_reuses_nothing():
    rng = np.random.default_rng(1)
    m = Model(5, rng, cold=True)
    assert not any(m.step(np.zeros(5, np.int64)))
    assert all(t.reused_total == 0 for t in m.reuse)
    # sorted now: the same step again is refilled in place
    held = [len(Model._rows_of(m.plain[0], w)) for w in range(5)]
    assert m.step(np.zeros(5, np.int64))[0] is (sum(held) > 0)


def test_a_fifth_archetype_gets_no_record():
    rng = np.random.default_rng(2)
    m = Model(3, rng, cold=False)
    for w in range(3):      # every table holds a row of every world
        for t in m.plain + m.reuse:
            if len(Model._rows_of(t, w)) == 0:
                t.append(w, -1 - w)
    for t in m.plain + m.reuse:
        t.world_sort(3)
    skipped = m.step(np.full(3, 6))
    assert skipped == [True, True, True, True, False]
    assert m.reuse[4].reused_total == 0 and m.reuse[3].reused_total == 3
