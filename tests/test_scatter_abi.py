"""CPU-only: the surface of entity scatters exists at every layer -- the C ABI
(include/mwhip.h, added under ABI 9, exported by libmadrona_hip.so), the C++
members of <madrona/mw_gpu.hpp> (compiled in a conformance translation unit of
their own, for the host and for gfx950: tests/shims/scatter_conformance*) and the
Python wrapper (madrona_amd.simlib)."""
import ctypes as C
import inspect
import os
import re
import subprocess

from madrona_amd import scatter_ref, simlib
from madrona_amd.simlib import HIP_BUILD_DIR, REPO_ROOT

SCATTER_FUNCTIONS = ["mwhip_scatter_create", "mwhip_scatter_destroy", "mwhip_scatter_apply",
                     "mwhip_scatter_apply_async", "mwhip_scatter_buffer", "mwhip_scatter_select",
                     "mwhip_scatter_archetypes", "mwhip_scatter_worlds", "mwhip_scatter_written",
                     "mwhip_set_step_scatter"]


def _header():
    return open(os.path.join(REPO_ROOT, "include", "mwhip.h")).read()


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_ten_functions_and_the_two_limits():
    code = _code(_header())
    E, U32, U64 = r"mwhip_exec\s*\*\s*\w*", r"uint32_t\s+\w+", r"uint64_t\s+\w+"
    for pattern in (
            r"\bint\s+mwhip_scatter_create\s*\(\s*%s\s*,\s*const\s+mwhip_gather_source\s*\*\s*\w+"
            r"\s*,\s*const\s+uint32_t\s*\*\s*\w+\s*,\s*%s\s*,\s*uint64_t\s*\*\s*\w+\s*\)"
            % (E, U32),
            r"\bvoid\s+mwhip_scatter_destroy\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_scatter_apply\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_scatter_apply_async\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bvoid\s*\*\s*mwhip_scatter_buffer\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,"
            r"\s*uint64_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)" % (E, U64, U32),
            r"\bint32_t\s*\*\s*mwhip_scatter_select\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint32_t\s*\*\s*mwhip_scatter_archetypes\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint32_t\s*\*\s*mwhip_scatter_worlds\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint32_t\s*\*\s*mwhip_scatter_written\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_set_step_scatter\s*\(\s*%s\s*,\s*%s\s*,\s*int\s+\w+\s*\)" % (E, U64)):
        assert re.search(pattern, code), pattern
    assert re.search(r"#define\s+MWHIP_SCATTER_MAX_COLUMNS\s+32\b", code)
    assert re.search(r"#define\s+MWHIP_MAX_STEP_SCATTERS\s+8\b", code)


def test_header_still_says_abi_9_and_names_the_additions():
    line = re.search(r"#define\s+MWHIP_ABI_VERSION\s+(\d+u)(.*)", _header())
    assert line.group(1) == "9u"
    assert "mwhip_scatter_" in line.group(2) and "mwhip_set_step_scatter" in line.group(2)
    # (what was there stays named)
    assert "mwhip_gather_source" in line.group(2) and "mwhip_set_step_gather" in line.group(2)


def test_header_states_the_rule_and_warns_off_table_columns_as_a_source():
    text = " ".join(_header().split())
    section = text[text.index("Entity scatters (added under ABI 9)"):]
    section = " ".join(section[: section.index("#define MWHIP_SCATTER_MAX_COLUMNS")]
                       .replace(" * ", " ").split())
    for words in ("THE HIGHEST INDEX WINS", "column's own address is no source",
                  "a step scatter wins over a step write", "PREVIOUS replay",
                  "scatter N is not one of this executor's"):
        assert words in section, words


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "scatter_abi_check.c"
    src.write_text(
        '#include "mwhip.h"\n'
        "int main(void)\n{\n"
        "    uint64_t scatter = 0, bytes = 0;\n"
        "    uint32_t cell = 0, comps[2] = { 2, 3 };\n"
        "    mwhip_gather_source source = { &bytes, 1, 8, 0, 1, 0 };\n"
        "    int rc = mwhip_scatter_create(0, &source, comps,\n"
        "                                  2 < MWHIP_SCATTER_MAX_COLUMNS ? 2 : 0, &scatter);\n"
        "    rc |= mwhip_scatter_apply(0, scatter) | mwhip_scatter_apply_async(0, scatter);\n"
        "    rc |= mwhip_set_step_scatter(0, scatter, MWHIP_MAX_STEP_SCATTERS != 0);\n"
        "    rc |= mwhip_scatter_buffer(0, scatter, 0, &bytes, &cell) != 0;\n"
        "    rc |= mwhip_scatter_select(0, scatter) != (int32_t *)0;\n"
        "    rc |= mwhip_scatter_archetypes(0, scatter) != (int32_t *)0;\n"
        "    rc |= mwhip_scatter_worlds(0, scatter) != (int32_t *)0;\n"
        "    rc |= mwhip_scatter_written(0, scatter) != (int32_t *)0;\n"
        "    mwhip_scatter_destroy(0, scatter);\n"
        "    return rc;\n}\n")
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I",
                          os.path.join(REPO_ROOT, "include"), str(src), "-c", "-o",
                          str(tmp_path / "scatter_abi_check.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_runtime_exports_them(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    missing = [n for n in SCATTER_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing


def test_an_unknown_handle_is_refused_with_a_null_executor(built):
    """The lookup comes first: no executor (and no GPU) needed, and the message
    names the handle."""
    rt = simlib.runtime_lib()
    handle = 987654321
    for call in (lambda: rt.mwhip_scatter_apply(None, handle),
                 lambda: rt.mwhip_scatter_apply_async(None, handle),
                 lambda: rt.mwhip_set_step_scatter(None, handle, 1),
                 lambda: rt.mwhip_set_step_scatter(None, handle, 0)):
        assert call() == -3
        message = rt.mwhip_last_error().decode()
        assert "scatter %d is not one of this executor's" % handle in message, message
    nbytes, cell = C.c_uint64(7), C.c_uint32(7)
    assert rt.mwhip_scatter_buffer(None, handle, 0, C.byref(nbytes), C.byref(cell)) is None
    assert "scatter %d is not one of this executor's" % handle in rt.mwhip_last_error().decode()
    assert (nbytes.value, cell.value) == (7, 7)
    for fn in (rt.mwhip_scatter_select, rt.mwhip_scatter_archetypes, rt.mwhip_scatter_worlds,
               rt.mwhip_scatter_written):
        assert fn(None, handle) is None
        assert "scatter %d is not one of this executor's" % handle in \
            rt.mwhip_last_error().decode()
    rt.mwhip_scatter_destroy(None, handle)      # (harmless)
    out = C.c_uint64(5)
    comps = (C.c_uint32 * 1)(2)
    source = simlib.GatherSource(0x1000, 1, 8, 0, 1, 0)
    assert rt.mwhip_scatter_create(None, C.byref(source), comps, 1, C.byref(out)) != 0
    assert out.value == 5


def test_python_surface():
    params = inspect.signature(simlib.Simulator.entity_scatter).parameters
    assert list(params) == ["self", "source", "components"]
    assert issubclass(simlib.EntityScatter, simlib._ExecObject)
    assert not issubclass(simlib.EntityScatter, simlib.EntityGather)
    for member in ("apply", "apply_async", "tensor", "buffer_ptr", "cell_bytes", "every_step",
                   "close", "__enter__", "__exit__"):
        assert callable(getattr(simlib.EntityScatter, member)), member
    for prop in ("select", "archetypes", "worlds", "written"):
        assert isinstance(inspect.getattr_static(simlib.EntityScatter, prop), property), prop
    assert not hasattr(simlib.EntityScatter, "compute")
    assert inspect.signature(simlib.EntityScatter.every_step).parameters["on"].default is True
    assert list(inspect.signature(simlib.EntityScatter.tensor).parameters) == [
        "self", "name", "dtype"]
    assert list(inspect.signature(scatter_ref.scatter_ref).parameters) == [
        "handles", "select", "tables", "inputs"]


class _RefSim(simlib.Simulator):
    """A reference-backend simulator without a library."""

    def __init__(self):
        self.backend = "ref_cpu"
        self.handle = None
        self.num_worlds = 2
        self._scatters = []
        self._columns = [("T.A", 4, False)]


def test_reference_backend_refuses():
    sim = _RefSim()
    try:
        sim.entity_scatter((0x1000, 1, 8, 0, 1), ["A"])
    except RuntimeError as err:
        assert "HIP backend" in str(err)
    else:
        raise AssertionError("an entity scatter on the reference backend")
    assert sim._scatters == []


def test_cxx_surface_compiles_for_host_and_gfx950(built):
    """libscatter_conformance.so is linked from a host translation unit and a HIP
    one compiled for gfx950 that both name makeEntityScatter(), setStepScatter()
    and every member of MWHipEntityScatter; both saw the header's limits."""
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libscatter_conformance.so"))
    for prefix in ("scatterconf_host", "scatterconf_hip"):
        traits = getattr(lib, prefix + "_traits")
        traits.restype = C.c_uint32
        assert traits() == 0b11111, prefix      # move-only
        got = getattr(lib, prefix + "_caps")
        got.restype = C.c_uint32
        assert got() == (32 << 16 | 8), prefix
        assert hasattr(lib, prefix + "_cycle"), prefix
    with open(os.path.join(HIP_BUILD_DIR, "libscatter_conformance.so"), "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"scatterconfTouch" in blob
    inl = open(os.path.join(REPO_ROOT, "tests", "shims", "scatter_conformance.inl")).read()
    for member in ("exec->makeEntityScatter(", "exec->setStepScatter(", ".apply()",
                   ".applyAsync()", ".columnTensor(", ".selectTensor()", ".archetypesTensor()",
                   ".worldsTensor()", ".writtenTensor()", ".numHandles()",
                   "MWHIP_ABI_VERSION == 9u"):
        assert member in inl, member
