"""Entity scatters in numpy: the definition that mwhip_scatter_* (include/mwhip.h,
csrc/entity_scatter.hip) computes on the device, and the
yardstick of its tests.

The source of the N handles and the rule by which handle i NAMES row r of
table a are gather_ref.py's (read_handles, Table): id >= 0, 0 <= r < rows(a),
the row's Entity cell equals the handle bit for bit, its WorldID cell is not
-1; the first table in the order given and the lowest row win where tables
break uniqueness.  With `select` int32 [N] and per listed component c an input
in_c uint8 [N, cell_bytes], an apply is the sequential loop

    for i in range(N):
        if select[i] != 0 and handle i names (a, r):
            for every listed c that table a has a column of:
                column_c(a)[r] = in_c[i]

so among selected handles that name the same entity the HIGHEST INDEX wins, as
`column[rows] = values` assigned one at a time.  It leaves

    archetype[i]  = a, or -1 when handle i names nothing (whatever select says)
    world[i]      = that row's WorldID cell, or -1 likewise
    written[i]    = 1 exactly when select[i] != 0, handle i names an entity and
                    no selected handle of higher index names the same entity
                    (also when table a has none of the listed columns), else 0

and every other byte of every table as it was.  Like gather_ref.py this is a
statement about the TABLES alone: it searches them and knows no entity store.
"""
from __future__ import annotations

from typing import Dict, List, Mapping, Sequence, Tuple

import numpy as np

from .gather_ref import Table, _entity_words


def scatter_ref(handles, select, tables: Sequence[Table], inputs: Mapping[str, np.ndarray]
                ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, List[Table]]:
    """handles: uint32 [N, 2] (read_handles) or uint8 [N, 8]; select: int [N];
    tables: every table a handle may name, each with the listed columns it has
    (and any others: they come back unchanged); inputs: {component name: uint8
    [N, cell_bytes]}.  Returns (archetype int32 [N], world int32 [N], written
    int32 [N], the tables after the apply: copies, in the order given)."""
    handles = _entity_words(handles)
    n = handles.shape[0]
    select = np.asarray(select).ravel()
    if select.shape[0] != n:
        raise ValueError(f"scatter_ref: {n} handles, {select.shape[0]} select words")
    cells: Dict[str, np.ndarray] = {}
    for name, values in inputs.items():
        values = np.ascontiguousarray(values, dtype=np.uint8)
        if values.ndim != 2 or values.shape[0] != n:
            raise ValueError(f"scatter_ref: input {name!r} of shape {values.shape}, {n} handles")
        cells[name] = values

    after = [Table(t.archetype, t.entities, t.world_ids,
                   {name: column.copy() for name, column in t.columns.items()})
             for t in tables]
    for table in after:
        for name, values in cells.items():
            column = table.columns.get(name)
            if column is not None and column.shape[1] != values.shape[1]:
                raise ValueError(f"scatter_ref: table {table.archetype}: {name!r} has cells of "
                                 f"{column.shape[1]} bytes, {values.shape[1]} given")

    # (gen, id) -> (table, row): the first table and the lowest row win
    where: Dict[Tuple[int, int], Tuple[int, int]] = {}
    for t, table in enumerate(after):
        for row in np.flatnonzero(table.world_ids != -1).tolist():
            gen, ident = (int(v) for v in table.entities[row])
            if ident < 2 ** 31:         # (as int32: id >= 0)
                where.setdefault((gen, ident), (t, row))

    archetype = np.full(n, -1, dtype=np.int32)
    world = np.full(n, -1, dtype=np.int32)
    written = np.zeros(n, dtype=np.int32)
    last: Dict[Tuple[int, int], int] = {}
    for i in range(n):
        key = (int(handles[i, 0]), int(handles[i, 1]))
        hit = where.get(key)
        if hit is None:
            continue
        table = after[hit[0]]
        archetype[i] = table.archetype
        world[i] = table.world_ids[hit[1]]
        if select[i] == 0:
            continue
        for name, values in cells.items():
            column = table.columns.get(name)
            if column is not None:
                column[hit[1]] = values[i]
        last[key] = i
    written[list(last.values())] = 1
    return archetype, world, written, after
