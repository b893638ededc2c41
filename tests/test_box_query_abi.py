"""CPU-only: the surface of box queries exists at every layer -- the C ABI
(include/mwhip.h, added under ABI 9, exported by libmadrona_hip.so), the kernel's
place in the physics headers, and the Python wrapper (madrona_amd.simlib)."""
import ctypes as C
import inspect
import os
import re
import subprocess

from madrona_amd import box_ref, simlib
from madrona_amd.simlib import HIP_BUILD_DIR, REPO_ROOT

BOX_FUNCTIONS = ["mwhip_set_box_kernel", "mwhip_boxes_create", "mwhip_boxes_destroy",
                 "mwhip_boxes_compute", "mwhip_boxes_compute_async", "mwhip_boxes_buffer",
                 "mwhip_set_step_boxes"]


def _header():
    return open(os.path.join(REPO_ROOT, "include", "mwhip.h")).read()


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _struct(code, name):
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), code, flags=re.S)
    assert body, name
    return re.findall(r"(\w+)\s*(?:\[\w+\])?\s*[;,]", body.group(1))


def test_header_declares_the_functions_the_structs_and_the_limits():
    code = _code(_header())
    E, U32, U64 = r"mwhip_exec\s*\*\s*\w*", r"uint32_t\s+\w+", r"uint64_t\s+\w+"
    for pattern in (
            r"\bint\s+mwhip_set_box_kernel\s*\(\s*%s\s*,\s*const\s+void\s*\*\s*\w+\s*\)" % E,
            r"\bint\s+mwhip_boxes_create\s*\(\s*%s\s*,\s*const\s+mwhip_boxes_desc\s*\*\s*\w+"
            r"\s*,\s*uint64_t\s*\*\s*\w+\s*\)" % E,
            r"\bvoid\s+mwhip_boxes_destroy\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_boxes_compute\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_boxes_compute_async\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bvoid\s*\*\s*mwhip_boxes_buffer\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,"
            r"\s*uint64_t\s*\*\s*\w+\s*\)" % (E, U64, U32),
            r"\bint\s+mwhip_set_step_boxes\s*\(\s*%s\s*,\s*%s\s*,\s*int\s+\w+\s*\)" % (E, U64)):
        assert re.search(pattern, code), pattern
    assert re.search(r"#define\s+MWHIP_MAX_STEP_BOXES\s+4\b", code)
    assert re.search(r"#define\s+MWHIP_BOXES_PACKED\s+1u\b", code)
    for name, value in (("OK", "0"), ("SKIPPED", r"\(-1\)"), ("BAD_WORLD", r"\(-2\)"),
                        ("BAD_BOX", r"\(-3\)")):
        assert re.search(r"#define\s+MWHIP_BOXES_%s\s+%s\s" % (name, value), code), name
    for k, name in enumerate(("WORLD", "CENTRE", "LO", "HI", "STATUS", "COUNT", "HITS")):
        assert re.search(r"#define\s+MWHIP_BOXES_BUF_%s\s+%du\b" % (name, k), code), name
    assert re.search(r"#define\s+MWHIP_BOXES_NUM_BUFS\s+7u\b", code)
    assert _struct(code, "mwhip_boxes_desc") == [
        "num_bundles", "boxes_per_bundle", "max_hits", "bundles_per_world", "flags", "pad_",
        "world", "count", "centre"]
    assert _struct(code, "mwhip_box_args") == ["num_plans", "pad_", "items", "plans"]
    plan = _struct(code, "mwhip_box_plan")
    assert "chunks_per_bundle" in plan and "max_hits" in plan


def test_header_still_says_abi_9_and_names_the_additions():
    line = re.search(r"#define\s+MWHIP_ABI_VERSION\s+(\d+u)(.*)", _header())
    assert line.group(1) == "9u"
    for word in ("mwhip_boxes_", "mwhip_set_step_boxes", "mwhip_set_box_kernel",
                 "mwhip_boxes_desc", "mwhip_box_args"):
        assert word in line.group(2), word
    assert "no struct a simulator library is compiled against changed" in line.group(2)


def test_header_says_what_a_box_sees():
    text = " ".join(_header().replace(" * ", " ").split())
    section = text[text.index("Box queries (added under ABI 9)"):]
    section = section[: section.index("#define MWHIP_MAX_STEP_BOXES")]
    for phrase in ("LAST BROADPHASE PASS left it", "NOT capped by max_hits",
                   "this simulator registered no box kernel", "-3 for an unknown handle",
                   "-10 for buffers", "pMin = centre[f] + lo[b]"):
        assert phrase in section, phrase
    inl = open(os.path.join(REPO_ROOT, "madrona_amd", "include", "madrona", "phys_impl",
                            "box_query.inl")).read()
    assert "boxQueryKernel" in inl and "checkEntityAABBsOverlap<maxBoxes>" in inl
    phys = open(os.path.join(REPO_ROOT, "madrona_amd", "include", "madrona", "physics.inl")).read()
    assert phys.index("#include <madrona/phys_impl/tree_query.inl>") < \
        phys.index("#include <madrona/phys_impl/ray_query.inl>") < \
        phys.index("#include <madrona/phys_impl/box_query.inl>")
    assert "#include <madrona/phys_impl/box_query.inl>" in phys
    assert "mwhip_set_box_kernel(builder.exec()" in phys


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "boxes_abi_check.c"
    src.write_text(
        '#include "mwhip.h"\n'
        "int main(void)\n{\n"
        "    uint64_t boxes = 0, bytes = 0;\n"
        "    mwhip_boxes_desc desc = { 2, 3, 16, 0, MWHIP_BOXES_PACKED, 0, { 0, 0, 0 },\n"
        "                              { 0, 0, 0 }, { &bytes, 12, 0 } };\n"
        "    mwhip_box_args args = { 0, 0, { 0 }, { 0 } };\n"
        "    mwhip_box_plan plan = { 0 };\n"
        "    int rc = mwhip_boxes_create(0, &desc, &boxes) | mwhip_set_box_kernel(0, 0);\n"
        "    rc |= mwhip_boxes_compute(0, boxes) | mwhip_boxes_compute_async(0, boxes);\n"
        "    rc |= mwhip_set_step_boxes(0, boxes, MWHIP_MAX_STEP_BOXES != 0);\n"
        "    rc |= mwhip_boxes_buffer(0, boxes, MWHIP_BOXES_BUF_HITS, &bytes) != 0;\n"
        "    rc |= MWHIP_BOXES_OK + MWHIP_BOXES_SKIPPED + MWHIP_BOXES_BAD_WORLD\n"
        "        + MWHIP_BOXES_BAD_BOX + (int)MWHIP_BOXES_NUM_BUFS + (int)args.num_plans\n"
        "        + (int)plan.num_bundles;\n"
        "    mwhip_boxes_destroy(0, boxes);\n"
        "    return rc + (int)sizeof(desc) - 72 + (int)sizeof(args) - 56\n"
        "        + (int)sizeof(plan) - 104;\n}\n")
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I",
                          os.path.join(REPO_ROOT, "include"), str(src), "-c", "-o",
                          str(tmp_path / "boxes_abi_check.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_struct_sizes_agree_with_python():
    assert C.sizeof(simlib.BoxesDesc) == 72
    assert [f[0] for f in simlib.BoxesDesc._fields_] == [
        "num_bundles", "boxes_per_bundle", "max_hits", "bundles_per_world", "flags", "pad_",
        "world", "count", "centre"]


def test_runtime_exports_them(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    missing = [n for n in BOX_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing


def test_every_simulator_with_a_broadphase_carries_the_kernel(built):
    """The kernel is compiled into the simulator's code object, for gfx950."""
    for sim, has in (("broadphase_only", True), ("escape_room_phys", True), ("hideseek", True),
                     ("ball_pit", True), ("cartpole", False)):
        with open(simlib.hip_lib_path(sim), "rb") as f:
            blob = f.read()
        assert (b"boxQueryKernel" in blob) == has, sim
        assert b"gfx950" in blob


def test_an_unknown_handle_is_refused_with_a_null_executor(built):
    """The lookup comes first: no executor (and no GPU) needed, and the message
    names the handle."""
    rt = simlib.runtime_lib()
    handle = 987654321
    for call in (lambda: rt.mwhip_boxes_compute(None, handle),
                 lambda: rt.mwhip_boxes_compute_async(None, handle),
                 lambda: rt.mwhip_set_step_boxes(None, handle, 1),
                 lambda: rt.mwhip_set_step_boxes(None, handle, 0)):
        assert call() == -3
        message = rt.mwhip_last_error().decode()
        assert "box query %d is not one of this executor's" % handle in message, message
    nbytes = C.c_uint64(7)
    assert rt.mwhip_boxes_buffer(None, handle, 0, C.byref(nbytes)) is None
    assert str(handle) in rt.mwhip_last_error().decode()
    assert nbytes.value == 7
    rt.mwhip_boxes_destroy(None, handle)      # (harmless)


def test_a_bad_descriptor_is_refused_without_an_executor(built):
    rt = simlib.runtime_lib()
    out = C.c_uint64(5)
    desc = simlib.BoxesDesc(2, 3, 16, 0, 0, 0)
    assert rt.mwhip_boxes_create(None, C.byref(desc), C.byref(out)) == -2
    assert rt.mwhip_boxes_create(None, None, C.byref(out)) == -2
    assert out.value == 5
    assert rt.mwhip_set_box_kernel(None, None) == -2


def test_python_surface():
    params = inspect.signature(simlib.Simulator.box_query).parameters
    assert list(params) == ["self", "bundles", "boxes_per_bundle", "max_hits", "world", "centre",
                            "bundles_per_world", "count", "packed"]
    assert [params[p].default for p in ("world", "centre", "bundles_per_world", "count",
                                        "packed")] == [None, None, 0, None, False]
    assert issubclass(simlib.BoxQuery, simlib._ExecObject)
    for member in ("worlds", "centres", "lo", "hi", "status", "counts", "hits", "handle_source",
                   "compute", "compute_async", "every_step", "close", "buffer_ptr", "__enter__",
                   "__exit__"):
        assert callable(getattr(simlib.BoxQuery, member)), member
    assert inspect.signature(simlib.BoxQuery.every_step).parameters["on"].default is True
    assert (simlib.BoxQuery.OK, simlib.BoxQuery.SKIPPED, simlib.BoxQuery.BAD_WORLD,
            simlib.BoxQuery.BAD_BOX) == \
        (box_ref.OK, box_ref.SKIPPED, box_ref.BAD_WORLD, box_ref.BAD_BOX)
    assert list(inspect.signature(box_ref.box_ref).parameters) == [
        "enumerate_world", "num_worlds", "bundles", "boxes_per_bundle", "max_hits", "lo", "hi",
        "centre", "world", "bundles_per_world", "count"]


class _RefSim(simlib.Simulator):
    """A reference-backend simulator without a library."""

    def __init__(self):
        self.backend = "ref_cpu"
        self.handle = None
        self.num_worlds = 2
        self._box_queries = []


def test_reference_backend_refuses():
    sim = _RefSim()
    try:
        sim.box_query(2, 3, 16)
    except RuntimeError as err:
        assert "HIP backend" in str(err)
    else:
        raise AssertionError("a box query on the reference backend")
    assert sim._box_queries == []


def test_cxx_surface_compiles_for_host_and_gfx950(built):
    """libboxes_conformance.so is linked from a host translation unit and a HIP
    one compiled for gfx950 that both name makeBoxQuery(), setStepBoxes() and
    every member of MWHipBoxQuery; both saw the header's limits and codes."""
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libboxes_conformance.so"))
    for prefix in ("boxesconf_host", "boxesconf_hip"):
        traits = getattr(lib, prefix + "_traits")
        traits.restype = C.c_uint32
        assert traits() == 0b11111, prefix      # move-only
        got = getattr(lib, prefix + "_caps")
        got.restype = C.c_uint32
        assert got() == (4 << 16 | 7 << 8 | 1 << 4 | 3), prefix
        assert hasattr(lib, prefix + "_cycle"), prefix
    with open(os.path.join(HIP_BUILD_DIR, "libboxes_conformance.so"), "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"boxesconfTouch" in blob
    inl = open(os.path.join(REPO_ROOT, "tests", "shims", "boxes_conformance.inl")).read()
    for member in ("exec->makeBoxQuery(", "exec->setStepBoxes(", ".compute()", ".computeAsync()",
                   ".worldsTensor()", ".centresTensor()", ".loTensor()", ".hiTensor()",
                   ".statusTensor()", ".countsTensor()", ".hitsTensor()", ".handleSource()",
                   ".numBundles()", ".numBoxes()", ".maxHits()", "MWHIP_ABI_VERSION == 9u"):
        assert member in inl, member
    text = open(os.path.join(REPO_ROOT, "madrona_amd", "include", "madrona", "mw_gpu.hpp")).read()
    assert "class MWHipBoxQuery : public detail::ExecObject<detail::BoxQueryKind>" in text
