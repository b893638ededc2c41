"""The state digest in numpy: the definition that the device kernel
(madrona_amd/csrc/digest.hip, mwhip_digest_* in include/mwhip.h)
reproduces bit for bit, and the yardstick of its tests.

A plan is an ordered list of columns, numbered by position p.  The columns of
one table form a group; a group's tag t is the plan position of its first
column.  All arithmetic is on uint64, modulo 2^64::

    fin(x):       x ^= x >> 30; x *= K2; x ^= x >> 27; x *= K3; x ^= x >> 31
    absorb(h, v): h = (h ^ v) * K1;  h ^= h >> 32
    row(g, r):    h = fin(t_g + K1)
                  for each column c of g in plan order:
                      h = absorb(h, p_c)
                      for each little-endian 32-bit word v of the cell
                              (zero-padded up to a multiple of 4 bytes):
                          h = absorb(h, v)
                  return fin(h)
    D[g][w] = sum of row(g, r) over the rows of g's table whose world is w

Rows whose world is negative (destroyed in place) add nothing.  The digest is
of the multiset of a world's rows: it does not see their order.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

K1 = np.uint64(0x9E3779B97F4A7C15)
K2 = np.uint64(0xBF58476D1CE4E5B9)
K3 = np.uint64(0x94D049BB133111EB)


def fin(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= K2
        x ^= x >> np.uint64(27)
        x *= K3
        x ^= x >> np.uint64(31)
    return x


def row_hashes(table_tag: int, cols: Sequence[Tuple[int, np.ndarray]]) -> np.ndarray:
    """cols: [(plan_index, uint8[rows, bytes])] of one group, in plan order;
    returns uint64[rows]."""
    n = cols[0][1].shape[0]
    with np.errstate(over="ignore"):
        h = np.full(n, fin(np.array([table_tag], np.uint64) + K1)[0], np.uint64)
        for tag, cells in cols:
            cells = np.asarray(cells, np.uint8).reshape(n, -1)
            pad = (-cells.shape[1]) % 4
            if pad:
                cells = np.concatenate([cells, np.zeros((n, pad), np.uint8)], axis=1)
            words = np.ascontiguousarray(cells).view("<u4").astype(np.uint64)
            h = (h ^ np.uint64(tag)) * K1
            h ^= h >> np.uint64(32)
            for j in range(words.shape[1]):
                h = (h ^ words[:, j]) * K1
                h ^= h >> np.uint64(32)
        return fin(h)


def group_digest(table_tag: int, cols: Sequence[Tuple[int, np.ndarray]],
                 world_of_row: np.ndarray, num_worlds: int) -> np.ndarray:
    """D[g]: uint64[num_worlds] of one group; world_of_row: int[rows], rows
    with a negative world (or one past num_worlds) add nothing."""
    world_of_row = np.asarray(world_of_row).astype(np.int64).reshape(-1)
    out = np.zeros(num_worlds, np.uint64)
    if world_of_row.size == 0:
        return out
    live = (world_of_row >= 0) & (world_of_row < num_worlds)
    hashes = row_hashes(table_tag, cols)
    with np.errstate(over="ignore"):
        np.add.at(out, world_of_row[live], hashes[live])
    return out


def plan_groups(keys: Sequence) -> List[Tuple[object, int, List[int]]]:
    """keys[p]: what identifies the table of plan column p (an archetype id or
    name).  Returns [(key, tag, [plan positions])] in group order."""
    groups: Dict[object, List[int]] = {}
    for p, key in enumerate(keys):
        groups.setdefault(key, []).append(p)
    return [(key, members[0], members) for key, members in groups.items()]


def digest_of_dump(keys: Sequence, columns: Sequence[Tuple[np.ndarray, np.ndarray]],
                   num_worlds: int) -> np.ndarray:
    """The digest of a plan from per-column dumps grouped by world
    (Simulator.dump_column): columns[p] = (uint8[rows, bytes], counts[worlds]).
    Returns uint64[groups, num_worlds]."""
    groups = plan_groups(keys)
    out = np.zeros((len(groups), num_worlds), np.uint64)
    for g, (_, tag, members) in enumerate(groups):
        counts = np.asarray(columns[members[0]][1]).astype(np.int64)
        world_of_row = np.repeat(np.arange(num_worlds), counts)
        out[g] = group_digest(tag, [(p, columns[p][0]) for p in members],
                              world_of_row, num_worlds)
    return out
