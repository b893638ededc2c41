"""CPU-only: the surface of world writes exists at every layer -- the C ABI
(include/mwhip.h, added under ABI 9, exported by libmadrona_hip.so), the C++
members of <madrona/mw_gpu.hpp> (compiled in a conformance translation unit of
their own, for the host and for gfx950: tests/shims/world_write_conformance*)
and the Python wrapper (madrona_amd.simlib)."""
import ctypes as C
import inspect
import os
import re
import subprocess

from madrona_amd import simlib, write_ref
from madrona_amd.simlib import HIP_BUILD_DIR, REPO_ROOT

WRITE_FUNCTIONS = ["mwhip_write_create", "mwhip_write_destroy", "mwhip_write_apply",
                   "mwhip_write_apply_async", "mwhip_write_buffer", "mwhip_write_take",
                   "mwhip_write_counts", "mwhip_set_step_write"]


def _header():
    return open(os.path.join(REPO_ROOT, "include", "mwhip.h")).read()


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_eight_functions_and_the_two_limits():
    code = _code(_header())
    E, U32, U64 = r"mwhip_exec\s*\*\s*\w*", r"uint32_t\s+\w+", r"uint64_t\s+\w+"
    for pattern in (
            r"\bint\s+mwhip_write_create\s*\(\s*%s\s*,\s*%s\s*,\s*const\s+uint32_t\s*\*\s*\w+"
            r"\s*,\s*%s\s*,\s*%s\s*,\s*uint64_t\s*\*\s*\w+\s*\)" % (E, U32, U32, U32),
            r"\bvoid\s+mwhip_write_destroy\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_write_apply\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_write_apply_async\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bvoid\s*\*\s*mwhip_write_buffer\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,"
            r"\s*uint64_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)" % (E, U64, U32),
            r"\bint32_t\s*\*\s*mwhip_write_take\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint32_t\s*\*\s*mwhip_write_counts\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_set_step_write\s*\(\s*%s\s*,\s*%s\s*,\s*int\s+\w+\s*\)" % (E, U64)):
        assert re.search(pattern, code), pattern
    assert re.search(r"#define\s+MWHIP_WRITE_MAX_COLUMNS\s+32\b", code)
    assert re.search(r"#define\s+MWHIP_MAX_STEP_WRITES\s+8\b", code)


def test_header_still_says_abi_9_and_names_the_additions():
    line = re.search(r"#define\s+MWHIP_ABI_VERSION\s+(\d+u)(.*)", _header())
    assert line.group(1) == "9u"
    assert "mwhip_write_" in line.group(2) and "mwhip_set_step_write" in line.group(2)
    # (and everything it named before)
    for earlier in ("mwhip_snapshot_", "mwhip_set_output_ring", "mwhip_digest_",
                    "mwhip_set_step_digest", "mwhip_view_", "mwhip_set_step_view"):
        assert earlier in line.group(2), earlier


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "write_abi_check.c"
    src.write_text(
        '#include "mwhip.h"\n'
        "int main(void)\n{\n"
        "    uint64_t write = 0, bytes = 0;\n"
        "    uint32_t cell = 0, comps[2] = { 2, 3 };\n"
        "    int rc = mwhip_write_create(0, 0, comps, 2, MWHIP_WRITE_MAX_COLUMNS, &write);\n"
        "    rc |= mwhip_write_apply(0, write) | mwhip_write_apply_async(0, write);\n"
        "    rc |= mwhip_set_step_write(0, write, MWHIP_MAX_STEP_WRITES != 0);\n"
        "    rc |= mwhip_write_buffer(0, write, 0, &bytes, &cell) != 0;\n"
        "    rc |= mwhip_write_take(0, write) != (int32_t *)0;\n"
        "    rc |= mwhip_write_counts(0, write) != (int32_t *)0;\n"
        "    mwhip_write_destroy(0, write);\n"
        "    return rc;\n}\n")
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I",
                          os.path.join(REPO_ROOT, "include"), str(src), "-c", "-o",
                          str(tmp_path / "write_abi_check.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_runtime_exports_them(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    missing = [n for n in WRITE_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing


def test_an_unknown_handle_is_refused_with_a_null_executor(built):
    """The lookup comes first: no executor (and no GPU) needed, -3, and the
    message names the handle."""
    rt = simlib.runtime_lib()
    handle = 987654321
    for call in (lambda: rt.mwhip_write_apply(None, handle),
                 lambda: rt.mwhip_write_apply_async(None, handle),
                 lambda: rt.mwhip_set_step_write(None, handle, 1),
                 lambda: rt.mwhip_set_step_write(None, handle, 0)):
        assert call() == -3
        message = rt.mwhip_last_error().decode()
        assert "write %d is not one of this executor's" % handle in message, message
    nbytes, cell = C.c_uint64(7), C.c_uint32(7)
    assert rt.mwhip_write_buffer(None, handle, 0, C.byref(nbytes), C.byref(cell)) is None
    assert str(handle) in rt.mwhip_last_error().decode()
    assert (nbytes.value, cell.value) == (7, 7)
    assert rt.mwhip_write_take(None, handle) is None
    assert rt.mwhip_write_counts(None, handle) is None
    rt.mwhip_write_destroy(None, handle)      # (harmless)
    out = C.c_uint64(5)
    comps = (C.c_uint32 * 1)(2)
    assert rt.mwhip_write_create(None, 0, comps, 1, 4, C.byref(out)) != 0
    assert out.value == 5


def test_python_surface():
    params = inspect.signature(simlib.Simulator.world_write).parameters
    assert list(params) == ["self", "table", "columns", "max_rows"]
    assert params["columns"].default is None
    assert issubclass(simlib.WorldWrite, simlib._ExecObject)
    for member in ("apply", "apply_async", "tensor", "buffer_ptr", "cell_bytes", "every_step",
                   "close", "__enter__", "__exit__"):
        assert callable(getattr(simlib.WorldWrite, member)), member
    for prop in ("take", "counts", "take_ptr"):
        assert isinstance(inspect.getattr_static(simlib.WorldWrite, prop), property), prop
    assert inspect.signature(simlib.WorldWrite.every_step).parameters["on"].default is True
    assert list(inspect.signature(simlib.WorldWrite.tensor).parameters) == ["self", "name", "dtype"]
    assert list(inspect.signature(write_ref.write_of_raw).parameters) == [
        "world_ids", "column_bytes", "padded", "take", "num_worlds", "max_rows"]
    # ordering the fills against the apply is the caller's: the docstring says so
    assert "CALLER" in simlib.WorldWrite.__doc__.upper()
    assert "synchronize" in simlib.WorldWrite.__doc__


class _RefSim(simlib.Simulator):
    """A reference-backend simulator without a library."""

    def __init__(self):
        self.backend = "ref_cpu"
        self.handle = None
        self.num_worlds = 2
        self._writes = []
        self._columns = [("T.A", 4, False)]


def test_reference_backend_refuses():
    sim = _RefSim()
    try:
        sim.world_write("T", max_rows=4)
    except RuntimeError as err:
        assert "HIP backend" in str(err)
    else:
        raise AssertionError("a world write on the reference backend")
    assert sim._writes == []


def test_cxx_surface_compiles_for_host_and_gfx950(built):
    """libworld_write_conformance.so is linked from a host translation unit and
    a HIP one compiled for gfx950 that both name makeWorldWrite(),
    setStepWrite() and every member of MWHipWorldWrite; both saw the header's
    limits."""
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    path = os.path.join(HIP_BUILD_DIR, "libworld_write_conformance.so")
    lib = C.CDLL(path)
    for prefix in ("writeconf_host", "writeconf_hip"):
        traits = getattr(lib, prefix + "_traits")
        traits.restype = C.c_uint32
        assert traits() == 0b11111, prefix      # move-only
        got = getattr(lib, prefix + "_caps")
        got.restype = C.c_uint32
        assert got() == (32 << 16 | 8), prefix
        assert hasattr(lib, prefix + "_cycle"), prefix
    with open(path, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"writeconfTouch" in blob
    inl = open(os.path.join(REPO_ROOT, "tests", "shims", "world_write_conformance.inl")).read()
    for member in ("exec->makeWorldWrite(", "exec->setStepWrite(", ".apply()", ".applyAsync()",
                   ".columnTensor(", ".takeTensor()", ".countsTensor()", ".maxRows()",
                   "MWHIP_ABI_VERSION == 9u"):
        assert member in inl, member


def test_the_runtime_is_built_from_the_kernel_and_the_shared_header():
    """world_write.hip is one of the runtime's sources, and world_team.hpp (the
    lane-level helpers it shares with world_view.hip) one of their dependencies."""
    makefile = open(os.path.join(REPO_ROOT, "madrona_amd", "Makefile")).read()
    srcs = re.search(r"RT_SRCS\s*:=((?:.*\\\n)*.*)", makefile).group(1)
    deps = re.search(r"RT_DEPS\s*:=((?:.*\\\n)*.*)", makefile).group(1)
    assert "csrc/world_write.hip" in srcs and "csrc/world_view.hip" in srcs
    assert "csrc/world_team.hpp" in deps
    csrc = os.path.join(REPO_ROOT, "madrona_amd", "csrc")
    for name in ("world_view.hip", "world_write.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "world_team.hpp"' in text, name
        assert "void teamCopy(" not in text and "void cellCopy(" not in text, name
