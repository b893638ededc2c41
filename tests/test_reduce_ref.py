"""CPU-only: madrona_amd/reduce_ref.py, the definition of world reductions in
numpy, against values worked out by hand on hand-made tables."""
import numpy as np
import pytest

from madrona_amd import reduce_ref
from madrona_amd.reduce_ref import Term, alarm_of, reduce_of_dump, reduce_of_raw

INF = np.float32(np.inf)
NAN = np.float32(np.nan)
DENORMAL = np.float32(1e-45)      # the smallest one: bits 0x00000001


def _f32(rows):
    """rows of floats -> uint8 [rows, 4 * elems]"""
    return np.asarray(rows, dtype=np.float32).reshape(len(rows), -1).view(np.uint8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _one(world_ids, cells, num_worlds, *term):
    result, counts = reduce_of_raw(np.asarray(world_ids, np.int32), cells, num_worlds,
                                   Term(*term))
    return result, counts


def test_the_float_sum_is_sequential_in_row_order():
    # (1e8 + 1) rounds to 1e8 in fp32: in row order the sum is 0; pairing the
    # outer two first, as a tree or a sort would, gives 1
    cells = _f32([[1e8], [1.0], [-1e8], [1e8], [-1e8], [1.0]])
    result, counts = _one([0, 0, 0, 1, 1, 1], cells, 2, "sum")
    assert result.dtype == np.float32 and result.shape == (2, 1)
    assert result[:, 0].tolist() == [0.0, 1.0]
    assert counts.tolist() == [3, 3] and counts.dtype == np.int32
    assert np.float32(1e8) + np.float32(1.0) == np.float32(1e8)
    # rows of a world are taken in table order wherever they are
    result, _ = _one([0, 1, 0, 1, 0, 1], _f32([[1e8], [1e8], [1.0], [-1e8], [-1e8], [1.0]]), 2,
                     "sum")
    assert result[:, 0].tolist() == [0.0, 1.0]


def test_a_denormal_survives_a_sum():
    result, _ = _one([0, 0, 1], _f32([[DENORMAL], [DENORMAL], [DENORMAL]]), 2, "sum")
    assert _bits(result)[:, 0].tolist() == [2, 1]
    # -0 into the +0 accumulator is +0
    result, _ = _one([0], _f32([[-0.0]]), 1, "sum")
    assert _bits(result)[0, 0] == 0


def test_signed_zero_ties_keep_the_first_one_met():
    for rows, want in (([[-0.0], [0.0]], 0x80000000), ([[0.0], [-0.0]], 0)):
        for op in ("min", "max"):
            result, _ = _one([0, 0], _f32(rows), 1, op)
            assert _bits(result)[0, 0] == want, (rows, op)


def test_nan_is_ignored_by_extrema_and_counted_by_both_counts():
    cells = _f32([[NAN], [2.0], [-3.0], [NAN]])
    ids = [0, 0, 0, 0]
    assert _one(ids, cells, 1, "min")[0][0, 0] == -3.0
    assert _one(ids, cells, 1, "max")[0][0, 0] == 2.0
    assert _one(ids, cells, 1, "absmax")[0][0, 0] == 3.0
    assert _one(ids, cells, 1, "count_nonzero")[0][0, 0] == 4
    assert _one(ids, cells, 1, "count_nonfinite")[0][0, 0] == 2
    assert np.isnan(_one(ids, cells, 1, "sum")[0][0, 0])
    # only NaNs: the identities stay
    only = _f32([[NAN], [NAN]])
    assert _one([0, 0], only, 1, "min")[0][0, 0] == INF
    assert _one([0, 0], only, 1, "max")[0][0, 0] == -INF
    assert _bits(_one([0, 0], only, 1, "absmax")[0])[0, 0] == 0


def test_inf_counts_in_absmax_and_minus_zero_is_not_nonzero():
    cells = _f32([[1.0, -0.0], [-INF, 0.0], [5.0, DENORMAL]])
    result, _ = _one([0, 0, 0], cells, 1, "absmax", "f32", 0, 2)
    assert result.dtype == np.float32
    assert result[0].tolist() == [np.inf, float(DENORMAL)]
    assert _one([0, 0, 0], cells, 1, "count_nonzero", "f32", 0, 2)[0][0].tolist() == [3, 1]
    assert _one([0, 0, 0], cells, 1, "count_nonfinite", "f32", 0, 2)[0][0].tolist() == [1, 0]
    assert _one([0, 0, 0], cells, 1, "min", "f32", 0, 2)[0][0].tolist() == [-np.inf, -0.0]


def test_u8_is_widened_and_offsets_and_elems_select_bytes():
    cells = np.array([[200, 1, 0, 9], [100, 2, 0, 9], [7, 3, 0, 9]], dtype=np.uint8)
    ids = [0, 0, 1]
    result, _ = _one(ids, cells, 2, "sum", "u8", 0, 3)
    assert result.dtype == np.uint32
    assert result.tolist() == [[300, 3, 0], [7, 3, 0]]
    assert _one(ids, cells, 2, "max", "u8", 0, 2)[0].tolist() == [[200, 2], [7, 3]]
    assert _one(ids, cells, 2, "min", "u8", 1, 1)[0].tolist() == [[1], [3]]
    nonzero, _ = _one(ids, cells, 2, "count_nonzero", "u8", 0, 4)
    assert nonzero.dtype == np.int32 and nonzero.tolist() == [[2, 2, 0, 2], [1, 1, 0, 1]]
    # the whole cell as one little-endian dword
    assert _one(ids, cells, 2, "max", "u32")[0].tolist() == [[0x09000264], [0x09000307]]


def test_integer_sums_wrap_and_extrema_are_signed_or_not():
    cells = np.array([[0xFFFFFFFF], [2], [0x80000000]], dtype=np.uint32).view(np.uint8)
    ids = [0, 0, 0]
    assert _one(ids, cells, 1, "sum", "u32")[0].tolist() == [[0x80000001]]
    signed, _ = _one(ids, cells, 1, "sum", "i32")
    assert signed.dtype == np.int32 and signed.tolist() == [[-(2 ** 31) + 1]]
    assert _one(ids, cells, 1, "max", "u32")[0].tolist() == [[0xFFFFFFFF]]
    assert _one(ids, cells, 1, "max", "i32")[0].tolist() == [[2]]
    assert _one(ids, cells, 1, "min", "u32")[0].tolist() == [[2]]
    assert _one(ids, cells, 1, "min", "i32")[0].tolist() == [[-(2 ** 31)]]


def test_an_empty_world_gets_the_identities():
    cells = _f32([[1.0]])
    for term, want in ((Term("sum"), 0), (Term("min"), 0x7F800000), (Term("max"), 0xFF800000),
                       (Term("absmax"), 0), (Term("count_nonzero"), 0),
                       (Term("count_nonfinite"), 0), (Term("sum", "u32"), 0),
                       (Term("min", "u32"), 0xFFFFFFFF), (Term("max", "u32"), 0),
                       (Term("min", "i32"), 0x7FFFFFFF), (Term("max", "i32"), 0x80000000),
                       (Term("min", "u8"), 0xFFFFFFFF), (Term("max", "u8"), 0)):
        result, counts = reduce_of_raw(np.array([1], np.int32), cells, 3, term)
        assert counts.tolist() == [0, 1, 0]
        assert _bits(result)[0, 0] == want and _bits(result)[2, 0] == want, term
    # a table without rows
    result, counts = reduce_of_raw(np.zeros(0, np.int32), np.zeros((0, 12), np.uint8), 2,
                                   Term("min", "f32", 0, 3))
    assert result.shape == (2, 3) and (result == INF).all() and not counts.any()


def test_holes_and_out_of_range_world_ids_are_skipped():
    cells = _f32([[1.0], [10.0], [100.0], [1000.0], [10000.0]])
    result, counts = _one([0, -1, 0, 2, 7], cells, 2, "sum")
    assert result[:, 0].tolist() == [101.0, 0.0] and counts.tolist() == [2, 0]
    # the world ids may come as their bytes
    ids = np.array([0, -1, 0, 2, 7], np.int32).view(np.uint8).reshape(5, 4)
    again, again_counts = reduce_of_raw(ids, cells, 2, Term("sum"))
    assert np.array_equal(again, result) and np.array_equal(again_counts, counts)


def test_reduce_of_dump_equals_reduce_of_raw():
    rng = np.random.default_rng(3)
    world_ids = rng.integers(-1, 5, size=200).astype(np.int32)
    cells = rng.integers(0, 256, size=(200, 12)).astype(np.uint8)
    order = np.argsort(world_ids, kind="stable")
    order = order[world_ids[order] >= 0]
    per_world = np.bincount(world_ids[world_ids >= 0], minlength=5)
    for term in (Term("sum", "f32", 0, 3), Term("absmax", "f32", 4, 2),
                 Term("count_nonfinite", "f32", 0, 3), Term("sum", "u8", 1, 11),
                 Term("min", "i32", 8, 1), Term("max", "u32", 0, 3),
                 Term("count_nonzero", "u8", 0, 12)):
        raw, raw_counts = reduce_of_raw(world_ids, cells, 5, term)
        dumped, dumped_counts = reduce_of_dump(cells[order], per_world, 5, term)
        assert raw.dtype == reduce_ref.result_dtype(term)
        assert np.array_equal(_bits(raw), _bits(dumped)), term
        assert np.array_equal(raw_counts, dumped_counts)
        assert raw_counts.tolist() == per_world.tolist()


def test_alarms():
    cells = _f32([[1.0, 2.0], [NAN, 0.0], [-7.0, 1.0], [3.0, INF]])
    ids = np.array([0, 1, 2, 3], np.int32)
    terms = [Term("count_nonfinite", "f32", 0, 2, 0.0, True),
             Term("absmax", "f32", 0, 2, 5.0, True),
             Term("min", "f32", 0, 2, 0.5, False)]
    results = [reduce_of_raw(ids, cells, 5, t)[0] for t in terms]
    # world 0: nothing; 1: NaN; 2: |-7| > 5; 3: Inf; 4: empty
    assert alarm_of(results, terms).tolist() == [0, 1, 1, 1, 0]
    assert alarm_of(results, [t._replace(alarm=False) for t in terms]).tolist() == [0] * 5
    low = Term("min", "f32", 0, 2, 0.5, True)
    assert alarm_of([reduce_of_raw(ids, cells, 5, low)[0]], [low]).tolist() == [0, 1, 1, 0, 0]
    high = Term("max", "f32", 0, 2, 2.5, True)
    assert alarm_of([reduce_of_raw(ids, cells, 5, high)[0]], [high]).tolist() == [0, 0, 0, 1, 0]


@pytest.mark.parametrize("term", [Term("absmax", "u32"), Term("count_nonfinite", "u8"),
                                  Term("sum", "f32", 0, 1, 0.0, True),
                                  Term("max", "u32", 0, 1, 0.0, True),
                                  Term("median"), Term("sum", "f64"), Term("sum", "f32", 0, 0),
                                  Term("sum", "f32", 2, 1), Term("sum", "f32", 0, 2)])
def test_what_the_definition_does_not_cover_raises(term):
    with pytest.raises(ValueError):
        reduce_of_raw(np.zeros(1, np.int32), np.zeros((1, 4), np.uint8), 1, term)


def test_the_constants_are_the_headers():
    import os
    import re

    from madrona_amd.simlib import REPO_ROOT
    header = open(os.path.join(REPO_ROOT, "include", "mwhip.h")).read()
    for name, value in [("F32", 0), ("I32", 1), ("U32", 2), ("U8", 3), ("ALARM", reduce_ref.ALARM),
                        ("MAX_TERMS", reduce_ref.MAX_TERMS), ("MAX_ELEMS", reduce_ref.MAX_ELEMS)]:
        assert re.search(r"#define\s+MWHIP_REDUCE_%s\s+%du?\b" % (name, value), header), name
        if name.lower() in reduce_ref.DTYPES:
            assert reduce_ref.DTYPES[name.lower()] == value
    for name, value in reduce_ref.OPS.items():
        assert re.search(r"#define\s+MWHIP_REDUCE_%s\s+%du\b" % (name.upper(), value), header)
    assert re.search(r"#define\s+MWHIP_MAX_STEP_REDUCES\s+%d\b" % reduce_ref.MAX_STEP_REDUCES,
                     header)
