"""Entity gathers in numpy: the definition that mwhip_gather_* (include/mwhip.h,
csrc/entity_gather.hip) computes on the device, and the
yardstick of its tests.

The SOURCE of handles is a run of records: `num_records` records of
`record_bytes` each, and in each record `handles_per_record` consecutive 8-byte
Entity cells ({uint32 gen; int32 id}, little endian) from byte `first_byte` on.
N = num_records * handles_per_record, and handle i is read at

    (i // handles_per_record) * record_bytes + first_byte + (i % handles_per_record) * 8

A handle h NAMES row r of table a exactly when h.id >= 0, a is one of the
tables given, 0 <= r < rows(a), the Entity cell of that row equals h bit for
bit, and the row's WorldID cell is not -1.  A handle with a negative id is no
entity's: Entity::none() is what the Entity cell of a row without an entity
holds (a temporary's, makeTemporary; a row destroyed in place, whose WorldID
cell is -1 as well), and it names none of them.  The ECS keeps the row a handle
names unique; given tables that break that, the first table in the order given
and the lowest row win.  Then

    archetype[i]  = a, or -1 when handle i names nothing
    world[i]      = that row's WorldID cell, or -1 likewise
    cells_c[i]    = the row's cell of component c; zero bytes when handle i
                    names nothing or table a has no column of c

This is a statement about the TABLES alone: the device kernel gets there through
the entity store without searching, this file searches and knows no store.
"""
from __future__ import annotations

from typing import Dict, Mapping, Sequence, Tuple

import numpy as np


class Table:
    """One table: `archetype` (what archetype[] reports), `entities` uint32
    [rows, 2] (gen, id), `world_ids` int32 [rows], `columns` {component:
    uint8 [rows, cell_bytes]}, all in one row order."""

    def __init__(self, archetype: int, entities, world_ids, columns: Mapping[str, np.ndarray]):
        self.archetype = int(archetype)
        self.entities = _entity_words(entities)
        world_ids = np.ascontiguousarray(world_ids)
        if world_ids.dtype == np.uint8:
            world_ids = world_ids.reshape(-1, 4).view("<i4")
        self.world_ids = world_ids.astype(np.int32).ravel()
        rows = self.entities.shape[0]
        if self.world_ids.shape[0] != rows:
            raise ValueError(f"table {archetype}: {rows} Entity cells, "
                             f"{self.world_ids.shape[0]} WorldID cells")
        self.columns: Dict[str, np.ndarray] = {}
        for name, cells in columns.items():
            cells = np.ascontiguousarray(cells, dtype=np.uint8)
            if cells.ndim != 2 or cells.shape[0] != rows:
                raise ValueError(f"table {archetype}: column {name!r} of shape {cells.shape}, "
                                 f"{rows} rows")
            self.columns[name] = cells


def _entity_words(cells) -> np.ndarray:
    """Entity cells as uint32 [n, 2]: from uint8 [n, 8] (a dump), or any
    4-byte integer type [n, 2]."""
    cells = np.ascontiguousarray(cells)
    if cells.dtype == np.uint8:
        return cells.reshape(-1, 8).view("<u4").reshape(-1, 2).copy()
    if cells.dtype.itemsize != 4 or cells.dtype.kind not in "iu":
        raise TypeError(f"Entity cells of type {cells.dtype}")
    return cells.reshape(-1, 2).view(np.uint32).copy()


def table_of_raw(archetype: int, entities, world_ids,
                 columns: Mapping[str, np.ndarray]) -> Table:
    """From table-order dumps (Simulator.dump_column_raw: destroyed rows
    included, their WorldID cell -1)."""
    return Table(archetype, entities, world_ids, columns)


def table_of_dump(archetype: int, entities: Tuple[np.ndarray, np.ndarray],
                  columns: Mapping[str, Tuple[np.ndarray, np.ndarray]]) -> Table:
    """From per-world dumps (Simulator.dump_column / dump_all on either backend:
    (rows grouped by world in world order, the rows of each world)); the
    reference CPU backend keeps a table per world and has no WorldID column, so
    a row's world is the group it is dumped in."""
    rows, counts = entities
    counts = np.asarray(counts, dtype=np.int64)
    world_ids = np.repeat(np.arange(counts.shape[0], dtype=np.int32), counts)
    return Table(archetype, rows, world_ids, {name: c[0] for name, c in columns.items()})


def read_handles(buf, num_records: int, record_bytes: int, first_byte: int = 0,
                 handles_per_record: int = 1) -> np.ndarray:
    """The N handles of a source whose bytes are `buf` (any array; read as
    bytes), as uint32 [N, 2] (gen, id)."""
    if handles_per_record < 1 or num_records < 1:
        raise ValueError("read_handles: no handles")
    if first_byte + 8 * handles_per_record > record_bytes:
        raise ValueError(f"read_handles: {handles_per_record} handles from byte {first_byte} "
                         f"do not fit a record of {record_bytes} bytes")
    raw = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    if raw.shape[0] < num_records * record_bytes:
        raise ValueError(f"read_handles: {raw.shape[0]} bytes, {num_records} records of "
                         f"{record_bytes}")
    records = raw[: num_records * record_bytes].reshape(num_records, record_bytes)
    cells = records[:, first_byte: first_byte + 8 * handles_per_record]
    return np.ascontiguousarray(cells).view("<u4").reshape(-1, 2).copy()


def gather_ref(handles, tables: Sequence[Table], components: Sequence[Tuple[str, int]]):
    """handles: uint32 [N, 2] (read_handles) or uint8 [N, 8]; tables: every
    table a handle may name; components: [(name, cell_bytes)].  Returns
    (archetype int32 [N], world int32 [N], {name: uint8 [N, cell_bytes]})."""
    handles = _entity_words(handles)
    n = handles.shape[0]
    archetype = np.full(n, -1, dtype=np.int32)
    world = np.full(n, -1, dtype=np.int32)
    cells = {name: np.zeros((n, int(size)), dtype=np.uint8) for name, size in components}
    if len(cells) != len(components):
        raise ValueError("gather_ref: a component is listed twice")
    keys = handles.view("<u8").ravel()
    is_entity = handles[:, 1].view(np.int32) >= 0
    for table in tables:
        live = np.flatnonzero(table.world_ids != -1)
        if live.size == 0:
            continue
        row_keys = table.entities.view("<u8").ravel()[live]
        order = np.argsort(row_keys, kind="stable")     # (lowest row first among equals)
        sorted_keys = row_keys[order]
        at = np.searchsorted(sorted_keys, keys, side="left")
        at_clipped = np.minimum(at, sorted_keys.shape[0] - 1)
        hit = (sorted_keys[at_clipped] == keys) & (archetype == -1) & is_entity
        idx = np.flatnonzero(hit)
        rows = live[order[at_clipped[idx]]]
        archetype[idx] = table.archetype
        world[idx] = table.world_ids[rows]
        for name, size in components:
            column = table.columns.get(name)
            if column is None:
                continue
            if column.shape[1] != int(size):
                raise ValueError(f"gather_ref: table {table.archetype}: {name!r} has cells of "
                                 f"{column.shape[1]} bytes, {size} listed")
            cells[name][idx] = column[rows]
    return archetype, world, cells
