"""World writes in numpy: the definition that mwhip_write_* (include/mwhip.h,
csrc/world_write.hip) applies on the device, and the yardstick of its tests.

A write is the inverse of a world view (view_ref.py): per listed column a
world-major tensor [worlds, max_rows, cell_bytes], plus an int32 `take` per
world.  With `world_ids` the table's WorldID column in TABLE ORDER (what
Simulator.dump_column_raw gives, destroyed rows included):

    count[w]  = number of rows r with world_ids[r] == w (not clipped)
    k[w]      = min(max(take[w], 0), count[w], max_rows)
    the cell of the j-th such row, ascending r, becomes padded[w, j] for j < k[w]

Every other cell is unchanged: rows of w from k[w] on, rows whose world id is
negative (destroyed in place) or not below num_worlds, which belong to no
world.  Nothing here depends on the table being sorted, and the inputs are not
modified.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np


def write_of_raw(world_ids, column_bytes, padded, take, num_worlds: int,
                 max_rows: int) -> Tuple[np.ndarray, np.ndarray]:
    """world_ids: int32 [rows] (or its bytes, uint8 [rows, 4]); column_bytes:
    uint8 [rows, cell_bytes] in the same order; padded: uint8 [num_worlds,
    max_rows, cell_bytes]; take: int32 [num_worlds].  Returns (the column after
    the write, uint8 [rows, cell_bytes], a new array; counts int32
    [num_worlds])."""
    if max_rows < 1:
        raise ValueError("write_of_raw: max_rows must be at least 1")
    world_ids = np.ascontiguousarray(world_ids)
    if world_ids.dtype == np.uint8:
        world_ids = world_ids.reshape(-1, 4).view(np.int32)
    world_ids = world_ids.astype(np.int64).ravel()
    cells = np.array(column_bytes, dtype=np.uint8, order="C")       # (a copy)
    if cells.ndim != 2 or cells.shape[0] != world_ids.shape[0]:
        raise ValueError(f"write_of_raw: {world_ids.shape[0]} world ids, "
                         f"column of shape {cells.shape}")
    padded = np.asarray(padded, dtype=np.uint8)
    if padded.shape != (num_worlds, max_rows, cells.shape[1]):
        raise ValueError(f"write_of_raw: padded of shape {padded.shape}, not "
                         f"{(num_worlds, max_rows, cells.shape[1])}")
    take = np.asarray(take).astype(np.int64).ravel()
    if take.shape != (num_worlds,):
        raise ValueError(f"write_of_raw: take of shape {take.shape}, {num_worlds} worlds")
    counts = np.zeros(num_worlds, dtype=np.int32)
    live = np.flatnonzero((world_ids >= 0) & (world_ids < num_worlds))
    # stable: a world's rows stay in table order
    live = live[np.argsort(world_ids[live], kind="stable")]
    worlds = world_ids[live]
    counts[:] = np.bincount(worlds, minlength=num_worlds)
    starts = np.cumsum(counts, dtype=np.int64) - counts
    rank = np.arange(len(live), dtype=np.int64) - starts[worlds]
    k = np.minimum(np.minimum(np.maximum(take, 0), counts), max_rows)
    keep = rank < k[worlds]
    cells[live[keep]] = padded[worlds[keep], rank[keep]]
    return cells, counts
