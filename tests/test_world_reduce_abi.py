"""CPU-only: the surface of world reduces exists at every layer -- the C ABI
(include/mwhip.h, added under ABI 9, exported by libmadrona_hip.so), the C++
members of <madrona/mw_gpu.hpp> (compiled in a conformance translation unit of
their own, for the host and for gfx950: tests/shims/reduce_conformance*) and
the Python wrapper (madrona_amd.simlib)."""
import ctypes as C
import inspect
import os
import re
import subprocess

from madrona_amd import reduce_ref, simlib
from madrona_amd.simlib import HIP_BUILD_DIR, REPO_ROOT

REDUCE_FUNCTIONS = ["mwhip_reduce_create", "mwhip_reduce_destroy", "mwhip_reduce_compute",
                    "mwhip_reduce_compute_async", "mwhip_reduce_buffer", "mwhip_reduce_counts",
                    "mwhip_reduce_alarm", "mwhip_set_step_reduce"]


def _header():
    return open(os.path.join(REPO_ROOT, "include", "mwhip.h")).read()


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_functions_the_term_and_the_limits():
    code = _code(_header())
    E, U32, U64 = r"mwhip_exec\s*\*\s*\w*", r"uint32_t\s+\w+", r"uint64_t\s+\w+"
    for pattern in (
            r"\bint\s+mwhip_reduce_create\s*\(\s*%s\s*,\s*%s\s*,\s*const\s+mwhip_reduce_term"
            r"\s*\*\s*\w+\s*,\s*%s\s*,\s*uint64_t\s*\*\s*\w+\s*\)" % (E, U32, U32),
            r"\bvoid\s+mwhip_reduce_destroy\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_reduce_compute\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_reduce_compute_async\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bvoid\s*\*\s*mwhip_reduce_buffer\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,"
            r"\s*uint64_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)" % (E, U64, U32),
            r"\bint32_t\s*\*\s*mwhip_reduce_counts\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint32_t\s*\*\s*mwhip_reduce_alarm\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_set_step_reduce\s*\(\s*%s\s*,\s*%s\s*,\s*int\s+\w+\s*\)" % (E, U64),
            r"typedef\s+struct\s+mwhip_reduce_term\s*\{\s*uint32_t\s+component_id\s*;\s*"
            r"uint32_t\s+byte_offset\s*;\s*uint32_t\s+num_elems\s*;\s*uint32_t\s+dtype\s*;\s*"
            r"uint32_t\s+op\s*;\s*uint32_t\s+flags\s*;\s*float\s+limit\s*;\s*\}"
            r"\s*mwhip_reduce_term\s*;"):
        assert re.search(pattern, code), pattern
    assert re.search(r"#define\s+MWHIP_REDUCE_MAX_TERMS\s+32\b", code)
    assert re.search(r"#define\s+MWHIP_REDUCE_MAX_ELEMS\s+256\b", code)
    assert re.search(r"#define\s+MWHIP_MAX_STEP_REDUCES\s+8\b", code)
    names = ["F32", "I32", "U32", "U8", "SUM", "MIN", "MAX", "ABSMAX", "COUNT_NONZERO",
             "COUNT_NONFINITE", "ALARM"]
    values = {n: re.search(r"#define\s+MWHIP_REDUCE_%s\s+(\d+)u\b" % n, code) for n in names}
    assert all(values.values()), values
    assert len({values[n].group(1) for n in names[:4]}) == 4
    assert len({values[n].group(1) for n in names[4:10]}) == 6
    assert values["ALARM"].group(1) == "1"
    # the definition is the header comment
    comment = _header()[_header().index("World reductions (added under ABI 9)"):]
    comment = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", comment[:comment.index("*/")]))
    for word in ("ascending r", "acc = acc + x_j in row order", "no flushing of denormals",
                 "A NaN never replaces", "the first one met stays", "exponent bits are all ones",
                 "gets the identities", "modulo 2^32", "256-byte aligned",
                 "reduce N is not one of this executor's"):
        assert word in comment, word


def test_header_still_says_abi_9_and_names_the_additions():
    line = re.search(r"#define\s+MWHIP_ABI_VERSION\s+(\d+u)(.*)", _header())
    assert line.group(1) == "9u"
    for name in ("mwhip_reduce_term", "mwhip_reduce_*()", "mwhip_set_step_reduce"):
        assert name in line.group(2), name


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "reduce_abi_check.c"
    src.write_text(
        '#include "mwhip.h"\n'
        "int main(void)\n{\n"
        "    uint64_t reduce = 0, bytes = 0;\n"
        "    uint32_t elems = 0;\n"
        "    mwhip_reduce_term terms[2] = {\n"
        "        { 2, 0, 3, MWHIP_REDUCE_F32, MWHIP_REDUCE_ABSMAX, MWHIP_REDUCE_ALARM, 100.0f },\n"
        "        { 3, 0, 1, MWHIP_REDUCE_U8, MWHIP_REDUCE_COUNT_NONZERO, 0, 0.0f } };\n"
        "    int rc = mwhip_reduce_create(0, 0, terms, 2, &reduce);\n"
        "    rc |= MWHIP_REDUCE_I32 + MWHIP_REDUCE_U32 + MWHIP_REDUCE_SUM + MWHIP_REDUCE_MIN +\n"
        "        MWHIP_REDUCE_MAX + MWHIP_REDUCE_COUNT_NONFINITE + MWHIP_REDUCE_MAX_TERMS +\n"
        "        MWHIP_REDUCE_MAX_ELEMS;\n"
        "    rc |= mwhip_reduce_compute(0, reduce) | mwhip_reduce_compute_async(0, reduce);\n"
        "    rc |= mwhip_set_step_reduce(0, reduce, MWHIP_MAX_STEP_REDUCES != 0);\n"
        "    rc |= mwhip_reduce_buffer(0, reduce, 0, &bytes, &elems) != 0;\n"
        "    rc |= mwhip_reduce_counts(0, reduce) != (int32_t *)0;\n"
        "    rc |= mwhip_reduce_alarm(0, reduce) != (int32_t *)0;\n"
        "    mwhip_reduce_destroy(0, reduce);\n"
        "    return rc;\n}\n")
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I",
                          os.path.join(REPO_ROOT, "include"), str(src), "-c", "-o",
                          str(tmp_path / "reduce_abi_check.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_runtime_exports_them(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    missing = [n for n in REDUCE_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing


def test_an_unknown_handle_is_refused_with_a_null_executor(built):
    """The lookup comes first: no executor (and no GPU) needed, and the message
    names the handle."""
    rt = simlib.runtime_lib()
    handle = 987654321
    for call in (lambda: rt.mwhip_reduce_compute(None, handle),
                 lambda: rt.mwhip_reduce_compute_async(None, handle),
                 lambda: rt.mwhip_set_step_reduce(None, handle, 1),
                 lambda: rt.mwhip_set_step_reduce(None, handle, 0)):
        assert call() != 0
        message = rt.mwhip_last_error().decode()
        assert "reduce %d is not one of this executor's" % handle in message, message
    nbytes, elems = C.c_uint64(7), C.c_uint32(7)
    assert rt.mwhip_reduce_buffer(None, handle, 0, C.byref(nbytes), C.byref(elems)) is None
    assert "reduce %d is not one of this executor's" % handle in rt.mwhip_last_error().decode()
    assert (nbytes.value, elems.value) == (7, 7)
    assert rt.mwhip_reduce_counts(None, handle) is None
    assert rt.mwhip_reduce_alarm(None, handle) is None
    assert "reduce %d is not one of this executor's" % handle in rt.mwhip_last_error().decode()
    rt.mwhip_reduce_destroy(None, handle)      # (harmless)
    out = C.c_uint64(5)
    terms = (simlib.ReduceTerm * 1)(simlib.ReduceTerm(0, 0, 1, 2, 0, 0, 0.0))
    assert rt.mwhip_reduce_create(None, 0, terms, 1, C.byref(out)) != 0
    assert out.value == 5


def test_python_surface():
    params = inspect.signature(simlib.Simulator.world_reduce).parameters
    assert list(params) == ["self", "table", "terms"]
    for member in ("compute", "compute_async", "tensor", "buffer_ptr", "every_step", "close",
                   "__enter__", "__exit__"):
        assert callable(getattr(simlib.WorldReduce, member)), member
    for member in ("counts", "alarm", "alarm_ptr"):
        assert isinstance(inspect.getattr_static(simlib.WorldReduce, member), property), member
    assert inspect.signature(simlib.WorldReduce.every_step).parameters["on"].default is True
    assert list(inspect.signature(simlib.WorldReduce.tensor).parameters) == ["self", "i"]
    assert issubclass(simlib.WorldReduce, simlib._ExecObject)
    assert simlib.WorldReduce._list == "_reduces"
    assert "_reduces" in inspect.getsource(simlib.Simulator.close)
    assert list(inspect.signature(reduce_ref.reduce_of_raw).parameters) == [
        "world_ids", "column_bytes", "num_worlds", "term"]
    assert list(inspect.signature(reduce_ref.reduce_of_dump).parameters) == [
        "rows", "counts", "num_worlds", "term"]
    # the ctypes mirror of mwhip_reduce_term
    assert C.sizeof(simlib.ReduceTerm) == 28
    assert [f[0] for f in simlib.ReduceTerm._fields_] == [
        "component_id", "byte_offset", "num_elems", "dtype", "op", "flags", "limit"]


class _RefSim(simlib.Simulator):
    """A reference-backend simulator without a library."""

    def __init__(self):
        self.backend = "ref_cpu"
        self.handle = None
        self.num_worlds = 2
        self._reduces = []
        self._columns = [("T.A", 4, False)]


def test_reference_backend_refuses():
    sim = _RefSim()
    try:
        sim.world_reduce("T", [("T.A", "sum")])
    except RuntimeError as err:
        assert "HIP backend" in str(err)
    else:
        raise AssertionError("a world reduce on the reference backend")
    assert sim._reduces == []


def test_cxx_surface_compiles_for_host_and_gfx950(built):
    """libreduce_conformance.so is linked from a host translation unit and a HIP
    one compiled for gfx950 that both name makeWorldReduce(), setStepReduce()
    and every member of MWHipWorldReduce; both saw the header's limits."""
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libreduce_conformance.so"))
    for prefix in ("reduceconf_host", "reduceconf_hip"):
        traits = getattr(lib, prefix + "_traits")
        traits.restype = C.c_uint32
        assert traits() == 0b11111, prefix      # move-only
        got = getattr(lib, prefix + "_caps")
        got.restype = C.c_uint32
        assert got() == (32 << 24 | 256 << 8 | 8), prefix
        assert hasattr(lib, prefix + "_cycle"), prefix
    with open(os.path.join(HIP_BUILD_DIR, "libreduce_conformance.so"), "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"reduceconfTouch" in blob
    inl = open(os.path.join(REPO_ROOT, "tests", "shims", "reduce_conformance.inl")).read()
    for member in ("exec->makeWorldReduce(", "exec->setStepReduce(", ".compute()",
                   ".computeAsync()", ".termTensor(", ".countsTensor()", ".alarmTensor()",
                   "MWHIP_ABI_VERSION == 9u"):
        assert member in inl, member
    # the runtime holds the kernel, compiled for gfx950
    with open(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), "rb") as f:
        assert b"worldReduceKernel" in f.read()
