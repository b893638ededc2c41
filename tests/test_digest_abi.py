"""CPU-only: the surface of state digests exists at every layer -- the C ABI
(include/mwhip.h, added under ABI 9, exported by libmadrona_hip.so), the C++
members of <madrona/mw_gpu.hpp> (compiled in a conformance translation unit of
their own, for the host and for gfx950: tests/shims/digest_conformance*), the
simulator C API and the Python wrapper (madrona_amd.simlib) -- and the numpy
definition (madrona_amd/digest_ref.py), the yardstick of
tests/test_digest_gpu.py, has the properties the digest is there for."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from madrona_amd import digest_ref, simlib
from madrona_amd.simlib import HIP_BUILD_DIR, REPO_ROOT

DIGEST_FUNCTIONS = ["mwhip_digest_create", "mwhip_digest_destroy", "mwhip_digest_compute",
                    "mwhip_digest_compute_async", "mwhip_digest_buffer", "mwhip_digest_group",
                    "mwhip_set_step_digest"]
# (the eighth name of the surface is the simulator's, sims/common/sim_c_api.h)
SIM_FUNCTION = "sim_hip_column_ids"


def _header():
    return open(os.path.join(REPO_ROOT, "include", "mwhip.h")).read()


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_headers_declare_the_eight_functions():
    code = _code(_header())
    E, U32, U64 = r"mwhip_exec\s*\*\s*\w*", r"uint32_t\s+\w+", r"uint64_t\s+\w+"
    P32 = r"uint32_t\s*\*\s*\w+"
    for pattern in (
            r"\bint\s+mwhip_digest_create\s*\(\s*%s\s*,\s*const\s+mwhip_digest_column\s*\*\s*\w+"
            r"\s*,\s*%s\s*,\s*uint64_t\s*\*\s*\w+\s*\)" % (E, U32),
            r"\bvoid\s+mwhip_digest_destroy\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_digest_compute\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_digest_compute_async\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bvoid\s*\*\s*mwhip_digest_buffer\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,\s*%s\s*\)"
            % (E, U64, P32, P32),
            r"\bint\s+mwhip_digest_group\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,\s*%s\s*,\s*%s\s*\)"
            % (E, U64, U32, P32, P32),
            r"\bint\s+mwhip_set_step_digest\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64)):
        assert re.search(pattern, code), pattern
    assert re.search(r"typedef\s+struct\s+mwhip_digest_column\s*\{\s*uint32_t\s+archetype_id\s*;"
                     r"\s*uint32_t\s+component_id\s*;\s*\}\s*mwhip_digest_column\s*;", code)
    # the caps are stated in the header
    assert re.search(r"#define\s+MWHIP_DIGEST_MAX_COLUMNS\s+\d+", code)
    assert re.search(r"#define\s+MWHIP_DIGEST_MAX_GROUPS\s+\d+", code)
    sim_api = _code(open(os.path.join(REPO_ROOT, "sims", "common", "sim_c_api.h")).read())
    assert re.search(r"\bint\s+sim_hip_column_ids\s*\(\s*SimHandle\s*\*\s*\w+\s*,\s*uint32_t\s+\w+"
                     r"\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)", sim_api)


def test_header_still_says_abi_9_and_names_the_additions():
    line = re.search(r"#define\s+MWHIP_ABI_VERSION\s+(\d+)u(.*)", _header())
    assert int(line.group(1)) == 9
    assert "mwhip_digest_" in line.group(2) and "mwhip_set_step_digest" in line.group(2)


def test_runtime_and_simulators_export_them(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    missing = [n for n in DIGEST_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing
    sim = C.CDLL(simlib.hip_lib_path("cartpole"), mode=C.RTLD_LOCAL)
    assert hasattr(sim, SIM_FUNCTION)


def test_an_unknown_handle_is_refused_with_a_null_executor(built):
    """The lookup comes first: no executor (and no GPU) needed, and the message
    names the handle."""
    rt = simlib.runtime_lib()
    handle = 987654321
    groups, worlds = C.c_uint32(7), C.c_uint32(7)
    for call in (lambda: rt.mwhip_digest_compute(None, handle),
                 lambda: rt.mwhip_digest_compute_async(None, handle),
                 lambda: rt.mwhip_set_step_digest(None, handle),
                 lambda: rt.mwhip_digest_group(None, handle, 0, C.byref(groups),
                                               C.byref(worlds))):
        assert call() != 0
        message = rt.mwhip_last_error().decode()
        assert "digest %d is not one of this executor's" % handle in message, message
    assert rt.mwhip_digest_buffer(None, handle, C.byref(groups), C.byref(worlds)) is None
    assert str(handle) in rt.mwhip_last_error().decode()
    assert (groups.value, worlds.value) == (7, 7)
    rt.mwhip_digest_destroy(None, handle)      # (harmless)
    # no columns: refused before the executor is looked at closely
    out = C.c_uint64(5)
    assert rt.mwhip_digest_create(None, None, 0, C.byref(out)) != 0
    assert out.value == 5


def test_python_surface():
    assert list(inspect.signature(simlib.Simulator.digest).parameters) == ["self", "columns"]
    assert inspect.signature(simlib.Simulator.digest).parameters["columns"].default is None
    for member in ("compute", "compute_async", "every_step", "close", "__enter__", "__exit__"):
        assert callable(getattr(simlib.StateDigest, member)), member
    assert isinstance(inspect.getattr_static(simlib.StateDigest, "tensor"), property)
    assert inspect.signature(simlib.StateDigest.every_step).parameters["on"].default is True
    assert simlib.DigestColumn._fields_ == [("archetype_id", C.c_uint32),
                                            ("component_id", C.c_uint32)]
    for name in ("K1", "K2", "K3", "fin", "row_hashes"):
        assert hasattr(digest_ref, name), name


class _RefSim(simlib.Simulator):
    """A reference-backend simulator with a dump list and no library: what
    StateDigest asks of a simulator whose backend has no executor."""

    def __init__(self, worlds, table):
        self.backend = "ref_cpu"
        self.handle = None
        self.num_worlds = worlds
        self._digests = []
        self._columns = [("T.A", 4, False), ("U.X", 1, False), ("T.B", 3, False)]
        self._table = table

    def dump_column(self, idx, max_rows_per_world=256):
        return self._table[idx]


def test_reference_backend_computes_and_refuses_the_rest():
    rng = np.random.default_rng(3)
    counts_t, counts_u = np.array([2, 0, 3], np.int32), np.array([1, 1, 0], np.int32)
    table = [(rng.integers(0, 256, (5, 4)).astype(np.uint8), counts_t),
             (rng.integers(0, 256, (2, 1)).astype(np.uint8), counts_u),
             (rng.integers(0, 256, (5, 3)).astype(np.uint8), counts_t)]
    sim = _RefSim(3, table)
    with sim.digest() as dig:
        assert dig.groups == ["T", "U"]
        D = dig.compute()
        assert D.dtype == np.uint64 and D.shape == (2, 3)
        worlds_t = np.repeat(np.arange(3), counts_t)
        expect_t = digest_ref.group_digest(0, [(0, table[0][0]), (2, table[2][0])], worlds_t, 3)
        expect_u = digest_ref.group_digest(1, [(1, table[1][0])], np.repeat(np.arange(3), counts_u), 3)
        assert np.array_equal(D, np.stack([expect_t, expect_u]))
        assert D[0, 1] == 0 and D[1, 2] == 0
        for call in (dig.compute_async, dig.every_step, lambda: dig.tensor):
            try:
                call()
            except RuntimeError as err:
                assert "HIP backend" in str(err)
            else:
                raise AssertionError("worked on the reference backend")
    assert sim._digests == []
    # names and indices select and order the plan
    with sim.digest(["T.B", 1]) as dig:
        assert dig.groups == ["T", "U"]
        assert np.array_equal(dig.compute()[0], digest_ref.group_digest(
            0, [(0, table[2][0])], np.repeat(np.arange(3), counts_t), 3))
    # Simulator.close() orphans what is open
    dig = sim.digest()
    sim.handle = None
    for d in sim._digests:
        d._orphan()
    try:
        dig.compute()
    except RuntimeError as err:
        assert "closed" in str(err)
    else:
        raise AssertionError("an orphaned digest computed")
    dig.close()     # (harmless)


# ---- the definition ---------------------------------------------------------------
def _one_world(tag, cols, rows=1):
    cols = [(p, np.tile(np.array(cell, np.uint8)[None, :], (rows, 1))) for p, cell in cols]
    return int(digest_ref.group_digest(tag, cols, np.zeros(rows, np.int64), 1)[0])


def test_known_answers():
    assert _one_world(0, [(0, [0, 0, 0, 0])]) == 0x56152ee5ccf33b4e
    assert _one_world(0, [(0, [0, 0, 0, 0])], rows=2) == 0xac2a5dcb99e6769c
    assert _one_world(0, [(0, [1, 2, 3])]) == 0xc08aeae8c3f10faa
    assert _one_world(0, [(0, [0xff]), (1, list(range(12)))]) == 0xd815fa92ac0063c8
    assert _one_world(2, [(2, [0xef, 0xbe, 0xad, 0xde, 1, 0, 0, 0]), (5, [7, 0])]) == \
        0xce6f8d2c27f2591b


def _random_table(rng, rows=300, worlds=7):
    cols = [(0, rng.integers(0, 256, (rows, 12)).astype(np.uint8)),
            (3, rng.integers(0, 256, (rows, 2)).astype(np.uint8)),
            (4, rng.integers(0, 256, (rows, 16)).astype(np.uint8))]
    return cols, rng.integers(0, worlds, rows), worlds


def test_invariant_under_a_row_permutation():
    rng = np.random.default_rng(0)
    cols, world, W = _random_table(rng)
    perm = rng.permutation(len(world))
    assert np.array_equal(
        digest_ref.group_digest(0, cols, world, W),
        digest_ref.group_digest(0, [(p, c[perm]) for p, c in cols], world[perm], W))


def test_one_flipped_bit_changes_exactly_one_world():
    rng = np.random.default_rng(1)
    cols, world, W = _random_table(rng)
    before = digest_ref.group_digest(0, cols, world, W)
    for c, row, byte, bit in ((0, 17, 11, 0), (1, 299, 1, 7), (2, 0, 0, 3)):
        flipped = [(p, cells.copy()) for p, cells in cols]
        flipped[c][1][row, byte] ^= np.uint8(1 << bit)
        after = digest_ref.group_digest(0, flipped, world, W)
        assert list(np.flatnonzero(after != before)) == [world[row]]


def test_a_cell_swapped_between_two_rows_of_one_world_is_seen():
    rng = np.random.default_rng(2)
    cols, world, W = _random_table(rng)
    a, b = np.flatnonzero(world == 4)[:2]
    swapped = [(p, cells.copy()) for p, cells in cols]
    swapped[1][1][[a, b]] = swapped[1][1][[b, a]]
    assert not np.array_equal(cols[1][1][a], cols[1][1][b])
    before = digest_ref.group_digest(0, cols, world, W)
    after = digest_ref.group_digest(0, swapped, world, W)
    assert list(np.flatnonzero(after != before)) == [4]


def test_rows_of_world_minus_one_are_ignored():
    rng = np.random.default_rng(4)
    cols, world, W = _random_table(rng)
    dead = rng.random(len(world)) < 0.3
    with_holes = np.where(dead, -1, world)
    assert np.array_equal(
        digest_ref.group_digest(0, cols, with_holes, W),
        digest_ref.group_digest(0, [(p, c[~dead]) for p, c in cols], world[~dead], W))
    assert not digest_ref.group_digest(0, cols, np.full(len(world), -1), W).any()


def test_short_cells_are_zero_padded():
    rng = np.random.default_rng(5)
    for width in (1, 2, 3):
        cells = rng.integers(1, 256, (9, width)).astype(np.uint8)
        padded = np.concatenate([cells, np.zeros((9, 4 - width), np.uint8)], axis=1)
        assert np.array_equal(digest_ref.row_hashes(0, [(0, cells)]),
                              digest_ref.row_hashes(0, [(0, padded)]))
    # ... at the end of the cell, not the front, and per cell, not per row
    assert _one_world(0, [(0, [1, 2, 3])]) != _one_world(0, [(0, [0, 1, 2, 3])])
    assert _one_world(0, [(0, [1]), (1, [2])]) != _one_world(0, [(0, [1, 2])])


def test_cxx_surface_compiles_for_host_and_gfx950(built):
    """libdigest_conformance.so is linked from a host translation unit and a HIP
    one compiled for gfx950 that both name makeDigest(), setStepDigest() and
    every member of MWHipDigest; both saw the header's caps."""
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libdigest_conformance.so"))
    code = _code(_header())
    caps = (int(re.search(r"#define\s+MWHIP_DIGEST_MAX_COLUMNS\s+(\d+)", code).group(1)) << 16 |
            int(re.search(r"#define\s+MWHIP_DIGEST_MAX_GROUPS\s+(\d+)", code).group(1)))
    for prefix in ("digconf_host", "digconf_hip"):
        traits = getattr(lib, prefix + "_traits")
        traits.restype = C.c_uint32
        assert traits() == 0b11111, prefix      # move-only
        got = getattr(lib, prefix + "_caps")
        got.restype = C.c_uint32
        assert got() == caps, prefix
        assert hasattr(lib, prefix + "_cycle"), prefix
    with open(os.path.join(HIP_BUILD_DIR, "libdigest_conformance.so"), "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"digconfTouch" in blob
    inl = open(os.path.join(REPO_ROOT, "tests", "shims", "digest_conformance.inl")).read()
    for member in ("exec->makeDigest(", "exec->setStepDigest(", ".compute()", ".computeAsync()",
                   ".devicePtr()", ".numGroups()"):
        assert member in inl, member
