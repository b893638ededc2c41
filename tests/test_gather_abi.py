"""CPU-only: the surface of entity gathers exists at every layer -- the C ABI
(include/mwhip.h, added under ABI 9, exported by libmadrona_hip.so), the C++
members of <madrona/mw_gpu.hpp> (compiled in a conformance translation unit of
their own, for the host and for gfx950: tests/shims/gather_conformance*) and the
Python wrapper (madrona_amd.simlib)."""
import ctypes as C
import inspect
import os
import re
import subprocess

from madrona_amd import gather_ref, simlib
from madrona_amd.simlib import HIP_BUILD_DIR, REPO_ROOT

GATHER_FUNCTIONS = ["mwhip_gather_create", "mwhip_gather_destroy", "mwhip_gather_compute",
                    "mwhip_gather_compute_async", "mwhip_gather_buffer",
                    "mwhip_gather_archetypes", "mwhip_gather_worlds", "mwhip_set_step_gather"]


def _header():
    return open(os.path.join(REPO_ROOT, "include", "mwhip.h")).read()


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_eight_functions_the_struct_and_the_two_limits():
    code = _code(_header())
    E, U32, U64 = r"mwhip_exec\s*\*\s*\w*", r"uint32_t\s+\w+", r"uint64_t\s+\w+"
    for pattern in (
            r"\bint\s+mwhip_gather_create\s*\(\s*%s\s*,\s*const\s+mwhip_gather_source\s*\*\s*\w+"
            r"\s*,\s*const\s+uint32_t\s*\*\s*\w+\s*,\s*%s\s*,\s*uint64_t\s*\*\s*\w+\s*\)"
            % (E, U32),
            r"\bvoid\s+mwhip_gather_destroy\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_gather_compute\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_gather_compute_async\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bvoid\s*\*\s*mwhip_gather_buffer\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,"
            r"\s*uint64_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)" % (E, U64, U32),
            r"\bint32_t\s*\*\s*mwhip_gather_archetypes\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint32_t\s*\*\s*mwhip_gather_worlds\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_set_step_gather\s*\(\s*%s\s*,\s*%s\s*,\s*int\s+\w+\s*\)" % (E, U64)):
        assert re.search(pattern, code), pattern
    assert re.search(r"#define\s+MWHIP_GATHER_MAX_COLUMNS\s+32\b", code)
    assert re.search(r"#define\s+MWHIP_MAX_STEP_GATHERS\s+8\b", code)
    struct = re.search(r"typedef\s+struct\s+mwhip_gather_source\s*\{(.*?)\}\s*mwhip_gather_source\s*;",
                       code, flags=re.S)
    assert struct, "mwhip_gather_source"
    names = re.findall(r"(\w+)\s*[;,]", struct.group(1))
    assert names == ["src", "num_records", "record_bytes", "first_byte", "handles_per_record",
                     "pad_"], names


def test_header_still_says_abi_9_and_names_the_additions():
    line = re.search(r"#define\s+MWHIP_ABI_VERSION\s+(\d+u)(.*)", _header())
    assert line.group(1) == "9u"
    assert "mwhip_gather_" in line.group(2) and "mwhip_set_step_gather" in line.group(2)
    assert "mwhip_gather_source" in line.group(2)


def test_header_warns_off_table_columns_as_a_source():
    text = " ".join(_header().split())
    section = text[text.index("Entity gathers (added under ABI 9)"):]
    section = section[: section.index("#define MWHIP_GATHER_MAX_COLUMNS")]
    assert "column's own address is NOT" in " ".join(section.replace(" * ", " ").split())
    assert "world view" in section


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "gather_abi_check.c"
    src.write_text(
        '#include "mwhip.h"\n'
        "int main(void)\n{\n"
        "    uint64_t gather = 0, bytes = 0;\n"
        "    uint32_t cell = 0, comps[2] = { 0, 1 };\n"
        "    mwhip_gather_source source = { &bytes, 1, 8, 0, 1, 0 };\n"
        "    int rc = mwhip_gather_create(0, &source, comps,\n"
        "                                 2 < MWHIP_GATHER_MAX_COLUMNS ? 2 : 0, &gather);\n"
        "    rc |= mwhip_gather_compute(0, gather) | mwhip_gather_compute_async(0, gather);\n"
        "    rc |= mwhip_set_step_gather(0, gather, MWHIP_MAX_STEP_GATHERS != 0);\n"
        "    rc |= mwhip_gather_buffer(0, gather, 0, &bytes, &cell) != 0;\n"
        "    rc |= mwhip_gather_archetypes(0, gather) != (int32_t *)0;\n"
        "    rc |= mwhip_gather_worlds(0, gather) != (int32_t *)0;\n"
        "    mwhip_gather_destroy(0, gather);\n"
        "    return rc + (int)sizeof(source) - 32;\n}\n")
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I",
                          os.path.join(REPO_ROOT, "include"), str(src), "-c", "-o",
                          str(tmp_path / "gather_abi_check.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_runtime_exports_them(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    missing = [n for n in GATHER_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing


def test_an_unknown_handle_is_refused_with_a_null_executor(built):
    """The lookup comes first: no executor (and no GPU) needed, and the message
    names the handle."""
    rt = simlib.runtime_lib()
    handle = 987654321
    for call in (lambda: rt.mwhip_gather_compute(None, handle),
                 lambda: rt.mwhip_gather_compute_async(None, handle),
                 lambda: rt.mwhip_set_step_gather(None, handle, 1),
                 lambda: rt.mwhip_set_step_gather(None, handle, 0)):
        assert call() == -3
        message = rt.mwhip_last_error().decode()
        assert "gather %d is not one of this executor's" % handle in message, message
    nbytes, cell = C.c_uint64(7), C.c_uint32(7)
    assert rt.mwhip_gather_buffer(None, handle, 0, C.byref(nbytes), C.byref(cell)) is None
    assert str(handle) in rt.mwhip_last_error().decode()
    assert (nbytes.value, cell.value) == (7, 7)
    assert rt.mwhip_gather_archetypes(None, handle) is None
    assert rt.mwhip_gather_worlds(None, handle) is None
    rt.mwhip_gather_destroy(None, handle)      # (harmless)
    out = C.c_uint64(5)
    comps = (C.c_uint32 * 1)(0)
    source = simlib.GatherSource(0x1000, 1, 8, 0, 1, 0)
    assert rt.mwhip_gather_create(None, C.byref(source), comps, 1, C.byref(out)) != 0
    assert out.value == 5


def test_python_surface():
    params = inspect.signature(simlib.Simulator.entity_gather).parameters
    assert list(params) == ["self", "source", "components"]
    assert issubclass(simlib.EntityGather, simlib._ExecObject)
    for member in ("compute", "compute_async", "tensor", "buffer_ptr", "cell_bytes", "every_step",
                   "close", "__enter__", "__exit__"):
        assert callable(getattr(simlib.EntityGather, member)), member
    for prop in ("archetypes", "worlds"):
        assert isinstance(inspect.getattr_static(simlib.EntityGather, prop), property), prop
    assert inspect.signature(simlib.EntityGather.every_step).parameters["on"].default is True
    assert list(inspect.signature(simlib.EntityGather.tensor).parameters) == [
        "self", "name", "dtype"]
    params = inspect.signature(simlib.WorldView.handle_source).parameters
    assert list(params) == ["self", "name", "first_byte", "handles"]
    assert (params["first_byte"].default, params["handles"].default) == (0, 1)
    assert list(inspect.signature(gather_ref.gather_ref).parameters) == [
        "handles", "tables", "components"]
    assert list(inspect.signature(gather_ref.read_handles).parameters) == [
        "buf", "num_records", "record_bytes", "first_byte", "handles_per_record"]
    assert C.sizeof(simlib.GatherSource) == 32
    assert [f[0] for f in simlib.GatherSource._fields_] == [
        "src", "num_records", "record_bytes", "first_byte", "handles_per_record", "pad_"]


class _RefSim(simlib.Simulator):
    """A reference-backend simulator without a library."""

    def __init__(self):
        self.backend = "ref_cpu"
        self.handle = None
        self.num_worlds = 2
        self._gathers = []
        self._columns = [("T.A", 4, False)]


def test_reference_backend_refuses():
    sim = _RefSim()
    try:
        sim.entity_gather((0x1000, 1, 8, 0, 1), ["A"])
    except RuntimeError as err:
        assert "HIP backend" in str(err)
    else:
        raise AssertionError("an entity gather on the reference backend")
    assert sim._gathers == []


class _TwoTables:
    """What EntityGather._component_id asks of a simulator: a dump list and
    sim_hip_column_ids."""

    def __init__(self, ids):
        self._columns = [(name, 4, False) for name in ids]
        self.handle = None
        outer = self

        class _Lib:
            @staticmethod
            def sim_hip_column_ids(handle, idx, arch, comp):
                arch._obj.value, comp._obj.value = outer._ids[idx]
                return 0
        self._ids = list(ids.values())
        self.lib = _Lib()


def test_a_component_name_must_mean_one_component():
    same = _TwoTables({"A.Entity": (3, 0), "A.Pos": (3, 7), "B.Pos": (4, 7), "B.Vel": (4, 9)})
    assert simlib.EntityGather._component_id(same, "Pos") == 7
    assert simlib.EntityGather._component_id(same, "Vel") == 9
    assert simlib.EntityGather._component_id(same, "Entity") == 0
    clash = _TwoTables({"A.Pos": (3, 7), "B.Pos": (4, 8)})
    for sim, name in ((clash, "Pos"), (same, "Rot"), (same, "A.Pos")):
        try:
            simlib.EntityGather._component_id(sim, name)
        except KeyError:
            pass
        else:
            raise AssertionError((name, "resolved"))


def test_cxx_surface_compiles_for_host_and_gfx950(built):
    """libgather_conformance.so is linked from a host translation unit and a HIP
    one compiled for gfx950 that both name makeEntityGather(), setStepGather()
    and every member of MWHipEntityGather; both saw the header's limits."""
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libgather_conformance.so"))
    for prefix in ("gatherconf_host", "gatherconf_hip"):
        traits = getattr(lib, prefix + "_traits")
        traits.restype = C.c_uint32
        assert traits() == 0b11111, prefix      # move-only
        got = getattr(lib, prefix + "_caps")
        got.restype = C.c_uint32
        assert got() == (32 << 16 | 8), prefix
        assert hasattr(lib, prefix + "_cycle"), prefix
    with open(os.path.join(HIP_BUILD_DIR, "libgather_conformance.so"), "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"gatherconfTouch" in blob
    inl = open(os.path.join(REPO_ROOT, "tests", "shims", "gather_conformance.inl")).read()
    for member in ("exec->makeEntityGather(", "exec->setStepGather(", ".compute()",
                   ".computeAsync()", ".columnTensor(", ".archetypesTensor()", ".worldsTensor()",
                   ".numHandles()", "MWHIP_ABI_VERSION == 9u"):
        assert member in inl, member
