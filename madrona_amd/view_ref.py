"""World views in numpy: the definition that mwhip_view_* (include/mwhip.h,
csrc/world_view.hip) computes on the device, and the yardstick of its tests.

A view of one table is, per listed column, a dense zero-padded world-major
copy [worlds, max_rows, cell_bytes] of the column's cells, plus an int32 count
per world.  With `world_ids` the table's WorldID column in TABLE ORDER (what
Simulator.dump_column_raw gives, destroyed rows included):

    count[w]        = number of rows r with world_ids[r] == w (not clipped)
    padded[w, j]    = the cell of the j-th such row, ascending r,
                      for j < min(count[w], max_rows)
    padded[w, j]    = zero bytes for the j from there up to max_rows

Rows whose world id is negative (destroyed in place) or not below num_worlds
belong to no world.  Nothing here depends on the table being sorted.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np


def view_of_raw(world_ids, column_bytes, num_worlds: int,
                max_rows: int) -> Tuple[np.ndarray, np.ndarray]:
    """world_ids: int32 [rows] (or its bytes, uint8 [rows, 4]); column_bytes:
    uint8 [rows, cell_bytes] in the same order.  Returns (padded uint8
    [num_worlds, max_rows, cell_bytes], counts int32 [num_worlds])."""
    if max_rows < 1:
        raise ValueError("view_of_raw: max_rows must be at least 1")
    world_ids = np.ascontiguousarray(world_ids)
    if world_ids.dtype == np.uint8:
        world_ids = world_ids.reshape(-1, 4).view(np.int32)
    world_ids = world_ids.astype(np.int64).ravel()
    cells = np.ascontiguousarray(column_bytes, dtype=np.uint8)
    if cells.ndim != 2 or cells.shape[0] != world_ids.shape[0]:
        raise ValueError(f"view_of_raw: {world_ids.shape[0]} world ids, "
                         f"column of shape {cells.shape}")
    padded = np.zeros((num_worlds, max_rows, cells.shape[1]), dtype=np.uint8)
    counts = np.zeros(num_worlds, dtype=np.int32)
    live = np.flatnonzero((world_ids >= 0) & (world_ids < num_worlds))
    # stable: a world's rows stay in table order
    live = live[np.argsort(world_ids[live], kind="stable")]
    worlds = world_ids[live]
    counts[:] = np.bincount(worlds, minlength=num_worlds)
    starts = np.cumsum(counts, dtype=np.int64) - counts
    rank = np.arange(len(live), dtype=np.int64) - starts[worlds]
    keep = rank < max_rows
    padded[worlds[keep], rank[keep]] = cells[live[keep]]
    return padded, counts


def view_of_dump(rows, counts, num_worlds: int, max_rows: int) -> Tuple[np.ndarray, np.ndarray]:
    """The same from a per-world dump (Simulator.dump_column on either backend:
    rows grouped by world in world order, uint8 [rows, cell_bytes], and the
    rows of each world)."""
    counts = np.asarray(counts, dtype=np.int64)
    world_ids = np.repeat(np.arange(num_worlds, dtype=np.int64), counts[:num_worlds])
    return view_of_raw(world_ids.astype(np.int32), rows, num_worlds, max_rows)
