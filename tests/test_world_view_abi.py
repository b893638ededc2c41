"""CPU-only: the surface of world views exists at every layer -- the C ABI
(include/mwhip.h, added under ABI 9, exported by libmadrona_hip.so), the C++
members of <madrona/mw_gpu.hpp> (compiled in a conformance translation unit of
their own, for the host and for gfx950: tests/shims/view_conformance*) and the
Python wrapper (madrona_amd.simlib)."""
import ctypes as C
import inspect
import os
import re
import subprocess

from madrona_amd import simlib, view_ref
from madrona_amd.simlib import HIP_BUILD_DIR, REPO_ROOT

VIEW_FUNCTIONS = ["mwhip_view_create", "mwhip_view_destroy", "mwhip_view_compute",
                  "mwhip_view_compute_async", "mwhip_view_buffer", "mwhip_view_counts",
                  "mwhip_set_step_view"]


def _header():
    return open(os.path.join(REPO_ROOT, "include", "mwhip.h")).read()


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_seven_functions_and_the_two_limits():
    code = _code(_header())
    E, U32, U64 = r"mwhip_exec\s*\*\s*\w*", r"uint32_t\s+\w+", r"uint64_t\s+\w+"
    for pattern in (
            r"\bint\s+mwhip_view_create\s*\(\s*%s\s*,\s*%s\s*,\s*const\s+uint32_t\s*\*\s*\w+"
            r"\s*,\s*%s\s*,\s*%s\s*,\s*uint64_t\s*\*\s*\w+\s*\)" % (E, U32, U32, U32),
            r"\bvoid\s+mwhip_view_destroy\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_view_compute\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_view_compute_async\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bvoid\s*\*\s*mwhip_view_buffer\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,"
            r"\s*uint64_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)" % (E, U64, U32),
            r"\bint32_t\s*\*\s*mwhip_view_counts\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_set_step_view\s*\(\s*%s\s*,\s*%s\s*,\s*int\s+\w+\s*\)" % (E, U64)):
        assert re.search(pattern, code), pattern
    assert re.search(r"#define\s+MWHIP_VIEW_MAX_COLUMNS\s+32\b", code)
    assert re.search(r"#define\s+MWHIP_MAX_STEP_VIEWS\s+8\b", code)


def test_header_still_says_abi_9_and_names_the_additions():
    line = re.search(r"#define\s+MWHIP_ABI_VERSION\s+(\d+u)(.*)", _header())
    assert line.group(1) == "9u"
    assert "mwhip_view_" in line.group(2) and "mwhip_set_step_view" in line.group(2)


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "view_abi_check.c"
    src.write_text(
        '#include "mwhip.h"\n'
        "int main(void)\n{\n"
        "    uint64_t view = 0, bytes = 0;\n"
        "    uint32_t cell = 0, comps[2] = { 0, 1 };\n"
        "    int rc = mwhip_view_create(0, 0, comps, 2, MWHIP_VIEW_MAX_COLUMNS, &view);\n"
        "    rc |= mwhip_view_compute(0, view) | mwhip_view_compute_async(0, view);\n"
        "    rc |= mwhip_set_step_view(0, view, MWHIP_MAX_STEP_VIEWS != 0);\n"
        "    rc |= mwhip_view_buffer(0, view, 0, &bytes, &cell) != 0;\n"
        "    rc |= mwhip_view_counts(0, view) != (int32_t *)0;\n"
        "    mwhip_view_destroy(0, view);\n"
        "    return rc;\n}\n")
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I",
                          os.path.join(REPO_ROOT, "include"), str(src), "-c", "-o",
                          str(tmp_path / "view_abi_check.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_runtime_exports_them(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    missing = [n for n in VIEW_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing


def test_an_unknown_handle_is_refused_with_a_null_executor(built):
    """The lookup comes first: no executor (and no GPU) needed, and the message
    names the handle."""
    rt = simlib.runtime_lib()
    handle = 987654321
    for call in (lambda: rt.mwhip_view_compute(None, handle),
                 lambda: rt.mwhip_view_compute_async(None, handle),
                 lambda: rt.mwhip_set_step_view(None, handle, 1),
                 lambda: rt.mwhip_set_step_view(None, handle, 0)):
        assert call() != 0
        message = rt.mwhip_last_error().decode()
        assert "view %d is not one of this executor's" % handle in message, message
    nbytes, cell = C.c_uint64(7), C.c_uint32(7)
    assert rt.mwhip_view_buffer(None, handle, 0, C.byref(nbytes), C.byref(cell)) is None
    assert str(handle) in rt.mwhip_last_error().decode()
    assert (nbytes.value, cell.value) == (7, 7)
    assert rt.mwhip_view_counts(None, handle) is None
    rt.mwhip_view_destroy(None, handle)      # (harmless)
    out = C.c_uint64(5)
    comps = (C.c_uint32 * 1)(0)
    assert rt.mwhip_view_create(None, 0, comps, 1, 4, C.byref(out)) != 0
    assert out.value == 5


def test_python_surface():
    params = inspect.signature(simlib.Simulator.world_view).parameters
    assert list(params) == ["self", "table", "columns", "max_rows"]
    assert params["columns"].default is None
    for member in ("compute", "compute_async", "tensor", "every_step", "close", "__enter__",
                   "__exit__"):
        assert callable(getattr(simlib.WorldView, member)), member
    assert isinstance(inspect.getattr_static(simlib.WorldView, "counts"), property)
    assert inspect.signature(simlib.WorldView.every_step).parameters["on"].default is True
    assert list(inspect.signature(simlib.WorldView.tensor).parameters) == ["self", "name", "dtype"]
    assert list(inspect.signature(view_ref.view_of_raw).parameters) == [
        "world_ids", "column_bytes", "num_worlds", "max_rows"]


class _RefSim(simlib.Simulator):
    """A reference-backend simulator without a library."""

    def __init__(self):
        self.backend = "ref_cpu"
        self.handle = None
        self.num_worlds = 2
        self._views = []
        self._columns = [("T.A", 4, False)]


def test_reference_backend_refuses():
    sim = _RefSim()
    try:
        sim.world_view("T", max_rows=4)
    except RuntimeError as err:
        assert "HIP backend" in str(err)
    else:
        raise AssertionError("a world view on the reference backend")
    assert sim._views == []


def test_cxx_surface_compiles_for_host_and_gfx950(built):
    """libview_conformance.so is linked from a host translation unit and a HIP
    one compiled for gfx950 that both name makeWorldView(), setStepView() and
    every member of MWHipWorldView; both saw the header's limits."""
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libview_conformance.so"))
    for prefix in ("viewconf_host", "viewconf_hip"):
        traits = getattr(lib, prefix + "_traits")
        traits.restype = C.c_uint32
        assert traits() == 0b11111, prefix      # move-only
        got = getattr(lib, prefix + "_caps")
        got.restype = C.c_uint32
        assert got() == (32 << 16 | 8), prefix
        assert hasattr(lib, prefix + "_cycle"), prefix
    with open(os.path.join(HIP_BUILD_DIR, "libview_conformance.so"), "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"viewconfTouch" in blob
    inl = open(os.path.join(REPO_ROOT, "tests", "shims", "view_conformance.inl")).read()
    for member in ("exec->makeWorldView(", "exec->setStepView(", ".compute()", ".computeAsync()",
                   ".columnTensor(", ".countsTensor()", ".maxRows()", "MWHIP_ABI_VERSION == 9u"):
        assert member in inl, member
