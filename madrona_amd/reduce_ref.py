"""World reductions in numpy: the definition that mwhip_reduce_*
(include/mwhip.h, csrc/world_reduce.hip) computes on the device, and the
yardstick of its tests.

A term reduces `elems` values of type `dtype` per row, found at byte `offset`
of a column's cell, over the rows of each world.  With `world_ids` the table's
WorldID column in TABLE ORDER (what Simulator.dump_column_raw gives, destroyed
rows included), the rows of world w are the rows r with world_ids[r] == w in
ascending r; rows whose world id is negative (destroyed in place) or not below
num_worlds belong to no world.  x_j is the value of the j-th such row:

    sum              f32: acc = +0.0, then acc = acc + x_j in row order, one
                     fp32 addition each (round to nearest, denormals kept);
                     integers: modulo 2^32 (u8 widened to u32)
    min              acc = +inf / the largest value of the result type;
                     if x_j < acc: acc = x_j  (a NaN never replaces; of -0 and
                     +0 the first one met stays)
    max              mirrored: acc = -inf / INT32_MIN / 0; if x_j > acc
    absmax           f32 only: acc = +0; a = x_j with the sign bit cleared;
                     if a > acc: acc = a  (NaNs are ignored, Inf counts)
    count_nonzero    int32: rows with x_j != 0 (NaN counts, -0 does not)
    count_nonfinite  f32 only, int32: rows whose exponent bits are all ones

A world without rows gets the identities.  An alarm term trips for a world
when any of its elements has count > 0, absmax / max > limit or min < limit;
alarm[w] is 1 if any alarm term trips.

The float sum is an explicit loop over row ranks, vectorised over worlds and
masked by j < count: np.sum would add pairwise.
"""
from __future__ import annotations

from typing import NamedTuple, Sequence, Tuple

import numpy as np

# the values of include/mwhip.h
DTYPES = {"f32": 0, "i32": 1, "u32": 2, "u8": 3}
OPS = {"sum": 0, "min": 1, "max": 2, "absmax": 3, "count_nonzero": 4, "count_nonfinite": 5}
ALARM = 1
MAX_TERMS, MAX_ELEMS, MAX_STEP_REDUCES = 32, 256, 8

_NUMPY = {"f32": np.float32, "i32": np.int32, "u32": np.uint32, "u8": np.uint8}
_RESULT = {"f32": np.float32, "i32": np.int32, "u32": np.uint32, "u8": np.uint32}


class Term(NamedTuple):
    op: str
    dtype: str = "f32"
    offset: int = 0
    elems: int = 1
    limit: float = 0.0
    alarm: bool = False


def result_dtype(term: Term) -> np.dtype:
    if term.op in ("count_nonzero", "count_nonfinite"):
        return np.dtype(np.int32)
    if term.op == "absmax":
        return np.dtype(np.float32)
    return np.dtype(_RESULT[term.dtype])


def _check(term: Term) -> None:
    if term.op not in OPS or term.dtype not in DTYPES:
        raise ValueError(f"reduce_ref: unknown op or dtype in {term}")
    if term.op in ("absmax", "count_nonfinite") and term.dtype != "f32":
        raise ValueError(f"reduce_ref: {term.op} needs f32 elements")
    if term.elems < 1:
        raise ValueError("reduce_ref: elems must be at least 1")
    if term.alarm and not (term.op.startswith("count_") or
                           (term.dtype == "f32" and term.op in ("min", "max", "absmax"))):
        raise ValueError(f"reduce_ref: an alarm has no rule for {term.op} on {term.dtype}")


def _per_world(world_ids, values, num_worlds: int):
    """values [rows, elems] -> ([num_worlds, most, elems] in row order, zero
    padded, and counts int32 [num_worlds])"""
    counts = np.zeros(num_worlds, dtype=np.int32)
    live = np.flatnonzero((world_ids >= 0) & (world_ids < num_worlds))
    # stable: a world's rows stay in table order
    live = live[np.argsort(world_ids[live], kind="stable")]
    worlds = world_ids[live]
    counts[:] = np.bincount(worlds, minlength=num_worlds)
    starts = np.cumsum(counts, dtype=np.int64) - counts
    rank = np.arange(len(live), dtype=np.int64) - starts[worlds]
    most = int(counts.max()) if num_worlds else 0
    padded = np.zeros((num_worlds, most, values.shape[1]), dtype=values.dtype)
    padded[worlds, rank] = values[live]
    return padded, counts


def reduce_of_raw(world_ids, column_bytes, num_worlds: int,
                  term: Term) -> Tuple[np.ndarray, np.ndarray]:
    """world_ids: int32 [rows] (or its bytes, uint8 [rows, 4]); column_bytes:
    uint8 [rows, cell_bytes] in the same order.  Returns (result [num_worlds,
    term.elems] in result_dtype(term), counts int32 [num_worlds])."""
    term = Term(*term)
    _check(term)
    world_ids = np.ascontiguousarray(world_ids)
    if world_ids.dtype == np.uint8:
        world_ids = world_ids.reshape(-1, 4).view(np.int32)
    world_ids = world_ids.astype(np.int64).ravel()
    cells = np.ascontiguousarray(column_bytes, dtype=np.uint8)
    if cells.ndim != 2 or cells.shape[0] != world_ids.shape[0]:
        raise ValueError(f"reduce_of_raw: {world_ids.shape[0]} world ids, "
                         f"column of shape {cells.shape}")
    item = np.dtype(_NUMPY[term.dtype]).itemsize
    end = term.offset + term.elems * item
    if term.offset % item != 0 or end > cells.shape[1]:
        raise ValueError(f"reduce_of_raw: {term} does not fit cells of {cells.shape[1]} bytes")
    values = np.ascontiguousarray(cells[:, term.offset:end]).view(_NUMPY[term.dtype])
    values = values.reshape(len(world_ids), term.elems)
    if term.dtype == "u8":
        values = values.astype(np.uint32)
    x, counts = _per_world(world_ids, values, num_worlds)
    shape = (num_worlds, term.elems)
    is_float = term.dtype == "f32"
    bits = x.view(np.uint32) if is_float else None

    op = term.op
    if op == "sum":
        # (integers: as uint32, which wraps)
        acc = np.zeros(shape, dtype=np.float32 if is_float else np.uint32)
        x = x if is_float else x.view(np.uint32)
    elif op == "min":
        acc = np.full(shape, np.inf if is_float else np.iinfo(x.dtype).max, dtype=x.dtype)
    elif op == "max":
        acc = np.full(shape, -np.inf if is_float else np.iinfo(x.dtype).min, dtype=x.dtype)
    elif op == "absmax":
        acc = np.zeros(shape, dtype=np.float32)
        x = (bits & np.uint32(0x7FFFFFFF)).view(np.float32)
    else:
        acc = np.zeros(shape, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(x.shape[1]):
            has = (j < counts)[:, None]
            xj = x[:, j]
            if op == "sum":
                acc = np.where(has, acc + xj, acc)
            elif op == "min":
                acc = np.where(has & (xj < acc), xj, acc)
            elif op in ("max", "absmax"):
                acc = np.where(has & (xj > acc), xj, acc)
            elif op == "count_nonzero":
                acc = acc + (has & (xj != 0)).astype(np.int32)
            else:
                nonfinite = (bits[:, j] & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
                acc = acc + (has & nonfinite).astype(np.int32)
    return np.ascontiguousarray(acc).view(result_dtype(term)).reshape(shape), counts


def reduce_of_dump(rows, counts, num_worlds: int, term: Term) -> Tuple[np.ndarray, np.ndarray]:
    """The same from a per-world dump (Simulator.dump_column on either backend:
    rows grouped by world in world order, uint8 [rows, cell_bytes], and the
    rows of each world)."""
    counts = np.asarray(counts, dtype=np.int64)
    world_ids = np.repeat(np.arange(num_worlds, dtype=np.int64), counts[:num_worlds])
    return reduce_of_raw(world_ids.astype(np.int32), rows, num_worlds, term)


def alarm_of(results: Sequence[np.ndarray], terms: Sequence[Term]) -> np.ndarray:
    """int32 [num_worlds]: 1 where a term with alarm=True trips.  results[i]
    is what reduce_of_raw gave for terms[i]."""
    alarm = np.zeros(len(results[0]), dtype=bool)
    with np.errstate(invalid="ignore"):
        for result, term in zip(results, terms):
            term = Term(*term)
            if not term.alarm:
                continue
            _check(term)
            if term.op.startswith("count_"):
                trips = result > 0
            elif term.op == "min":
                trips = result < np.float32(term.limit)
            else:
                trips = result > np.float32(term.limit)
            alarm |= trips.any(axis=1)
    return alarm.astype(np.int32)
