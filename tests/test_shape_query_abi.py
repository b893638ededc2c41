"""CPU-only: the surface of shape queries exists at every layer -- the C ABI
(include/mwhip.h, added under ABI 9, exported by libmadrona_hip.so), the kernel's
place in the physics headers and in the simulators' code objects, the C++
wrapper (madrona/mw_gpu.hpp) and the Python one (madrona_amd.simlib) -- and what
the C ABI refuses without an executor.  (What it refuses of a live executor is in
tests/test_shape_query_gpu.py: an executor needs the device.)"""
import ctypes as C
import inspect
import os
import re
import subprocess

from madrona_amd import shape_ref, simlib
from madrona_amd.simlib import HIP_BUILD_DIR, REPO_ROOT

SHAPE_FUNCTIONS = ["mwhip_set_shape_kernel", "mwhip_shapes_create", "mwhip_shapes_destroy",
                   "mwhip_shapes_compute", "mwhip_shapes_compute_async", "mwhip_shapes_buffer",
                   "mwhip_set_step_shapes"]
BUFS = ("WORLD", "EXCLUDE", "OBJECT", "POSITION", "ROTATION", "SCALE", "STATUS", "COUNT", "HITS",
        "SHAPE_IS_REF", "NUM_POINTS", "NORMAL", "POINTS")


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
            r"\bint\s+mwhip_set_shape_kernel\s*\(\s*%s\s*,\s*const\s+void\s*\*\s*\w+\s*,"
            r"\s*%s\s*\)" % (E, U32),
            r"\bint\s+mwhip_shapes_create\s*\(\s*%s\s*,\s*const\s+mwhip_shapes_desc\s*\*"
            r"\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)" % E,
            r"\bvoid\s+mwhip_shapes_destroy\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_shapes_compute\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_shapes_compute_async\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bvoid\s*\*\s*mwhip_shapes_buffer\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,"
            r"\s*uint64_t\s*\*\s*\w+\s*\)" % (E, U64, U32),
            r"\bint\s+mwhip_set_step_shapes\s*\(\s*%s\s*,\s*%s\s*,\s*int\s+\w+\s*\)" % (E, U64)):
        assert re.search(pattern, code), pattern
    assert re.search(r"#define\s+MWHIP_MAX_STEP_SHAPES\s+4\b", code)
    assert re.search(r"#define\s+MWHIP_SHAPES_PLAIN\s+1u\b", code)
    for name, value in (("OK", "0"), ("SKIPPED", r"\(-1\)"), ("BAD_WORLD", r"\(-2\)"),
                        ("BAD_SHAPE", r"\(-3\)"), ("UNSORTED", r"\(-4\)"),
                        ("UNSUPPORTED", r"\(-5\)")):
        assert re.search(r"#define\s+MWHIP_SHAPES_%s\s+%s\s" % (name, value), code), name
    for k, name in enumerate(BUFS):
        assert re.search(r"#define\s+MWHIP_SHAPES_BUF_%s\s+%du\b" % (name, k), code), name
    assert re.search(r"#define\s+MWHIP_SHAPES_NUM_BUFS\s+13u\b", code)
    assert _struct(code, "mwhip_shapes_desc") == [
        "num_bundles", "shapes_per_bundle", "max_hits", "num_objects", "bundles_per_world",
        "flags", "world", "count", "exclude"]
    assert _struct(code, "mwhip_shape_args") == ["num_plans", "pad_", "items", "plans"]
    plan = _struct(code, "mwhip_shape_plan")
    for field in ("state", "world_src", "count_src", "exclude_src", "object", "position",
                  "rotation", "scale", "status", "count", "hits", "shape_is_ref", "num_points",
                  "normal", "points", "scratch", "scratch_stride", "scratch_waves", "max_hits",
                  "num_objects", "bundles_per_world", "flags"):
        assert field in plan, field


def test_header_still_says_abi_9_and_names_the_additions():
    line = re.search(r"#define\s+MWHIP_ABI_VERSION\s+(\d+u)(.*)", _header())
    assert line.group(1) == "9u"
    for word in ("mwhip_shapes_", "mwhip_set_step_shapes", "mwhip_set_shape_kernel",
                 "mwhip_shapes_desc", "mwhip_shape_args"):
        assert word in line.group(2), word
    assert "no struct a simulator library is compiled against changed" in line.group(2)


def test_header_says_what_a_hit_is():
    text = " ".join(_header().replace(" * ", " ").split())
    section = text[text.index("Shape queries (added under ABI 9)"):]
    section = section[: section.index("#define MWHIP_MAX_STEP_SHAPES")]
    for phrase in ("is shape g of bundle f", "gen and id both", "Entity::none() excludes nothing",
                   "CURRENT Position, Rotation and Scale", "Static ones included",
                   "body_num_prims + bodyPrim", "ORDER: ascending (k, c)",
                   "No BVH is walked", "NOT capped by K", "No sticky error flag",
                   "in the order world, count, then per shape", "-3 for an unknown handle",
                   "-10 for buffers", "snapshots do not save them",
                   "The normal points away from the reference side"):
        assert phrase in section, phrase
    impl = os.path.join(REPO_ROOT, "madrona_amd", "include", "madrona")
    inl = open(os.path.join(impl, "phys_impl", "shape_query.inl")).read()
    for name in ("shapeQueryKernel", "collidePairLane(", "hullHullWave(", "collidePairStored(",
                 "WorldBodies bodies", "setupPair(", "Loc::none()"):
        assert name in inl, name
    # the stored path has a slot per wavefront, not the world's
    statements = re.sub(r"//[^\n]*", "", inl)
    assert "worldHullScratch" not in statements and "atomic" not in statements.lower()
    assert "__syncthreads" not in statements
    phys = open(os.path.join(impl, "physics.inl")).read()
    assert phys.index("#include <madrona/phys_impl/contact_query.inl>") < \
        phys.index("#include <madrona/phys_impl/shape_query.inl>")
    assert "mwhip_set_shape_kernel(builder.exec()" in phys
    # the step kernels and the contact kernel do not include the shared helper
    assert "query_store.inl" not in open(os.path.join(impl, "phys_impl",
                                                      "contact_query.inl")).read()
    launch = open(os.path.join(REPO_ROOT, "madrona_amd", "csrc", "runtime_launch.hip")).read()
    assert re.search(r"stepContactsStage,[^\n]*\n\s*stepShapesStage,[^\n]*\n\s*stepGatherStage,",
                     launch)


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "shapes_abi_check.c"
    src.write_text(
        '#include "mwhip.h"\n'
        "int main(void)\n{\n"
        "    uint64_t shapes = 0, bytes = 0;\n"
        "    mwhip_shapes_desc desc = { 4, 2, 8, 3, 0, MWHIP_SHAPES_PLAIN, { &bytes, 4, 0 },\n"
        "                               { 0, 0, 0 }, { &bytes, 8, 0 } };\n"
        "    mwhip_shape_args args = { 0, 0, { 0 }, { 0 } };\n"
        "    mwhip_shape_plan plan = { 0 };\n"
        "    int rc = mwhip_shapes_create(0, &desc, &shapes) | mwhip_set_shape_kernel(0, 0, 256);\n"
        "    rc |= mwhip_shapes_compute(0, shapes) | mwhip_shapes_compute_async(0, shapes);\n"
        "    rc |= mwhip_set_step_shapes(0, shapes, MWHIP_MAX_STEP_SHAPES != 0);\n"
        "    rc |= mwhip_shapes_buffer(0, shapes, MWHIP_SHAPES_BUF_HITS, &bytes) != 0;\n"
        "    rc |= MWHIP_SHAPES_OK + MWHIP_SHAPES_SKIPPED + MWHIP_SHAPES_BAD_WORLD\n"
        "        + MWHIP_SHAPES_BAD_SHAPE + MWHIP_SHAPES_UNSORTED + MWHIP_SHAPES_UNSUPPORTED\n"
        "        + (int)MWHIP_SHAPES_NUM_BUFS + (int)MWHIP_SHAPES_BUF_WORLD\n"
        "        + (int)MWHIP_SHAPES_BUF_EXCLUDE + (int)MWHIP_SHAPES_BUF_OBJECT\n"
        "        + (int)MWHIP_SHAPES_BUF_POSITION + (int)MWHIP_SHAPES_BUF_ROTATION\n"
        "        + (int)MWHIP_SHAPES_BUF_SCALE + (int)MWHIP_SHAPES_BUF_STATUS\n"
        "        + (int)MWHIP_SHAPES_BUF_COUNT + (int)MWHIP_SHAPES_BUF_SHAPE_IS_REF\n"
        "        + (int)MWHIP_SHAPES_BUF_NUM_POINTS + (int)MWHIP_SHAPES_BUF_NORMAL\n"
        "        + (int)MWHIP_SHAPES_BUF_POINTS + (int)args.num_plans + (int)plan.num_bundles;\n"
        "    mwhip_shapes_destroy(0, shapes);\n"
        "    return rc + (int)sizeof(desc) - 72 + (int)sizeof(args) - 56\n"
        "        + (int)sizeof(plan) - 176;\n}\n")
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I",
                          os.path.join(REPO_ROOT, "include"), str(src), "-c", "-o",
                          str(tmp_path / "shapes_abi_check.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_struct_sizes_agree_with_python():
    assert C.sizeof(simlib.ShapesDesc) == 72
    assert [f[0] for f in simlib.ShapesDesc._fields_] == [
        "num_bundles", "shapes_per_bundle", "max_hits", "num_objects", "bundles_per_world",
        "flags", "world", "count", "exclude"]
    assert [simlib.ShapeQuery._BUFS[name.lower()] for name in BUFS] == list(range(13))


def test_runtime_exports_them(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    missing = [n for n in SHAPE_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing


def test_every_simulator_with_a_rigid_body_step_carries_the_kernel(built):
    """The kernel is compiled into the simulator's code object, for gfx950."""
    for sim, has in (("contact_probe", True), ("escape_room_phys", True), ("hideseek", True),
                     ("ball_pit", True), ("tgs_drop", True), ("cartpole", False)):
        with open(simlib.hip_lib_path(sim), "rb") as f:
            blob = f.read()
        assert (b"shapeQueryKernel" in blob) == has, sim
        assert b"gfx950" in blob


def test_an_unknown_handle_is_refused_with_a_null_executor(built):
    """The lookup comes first: no executor (and no GPU) needed, and the message
    names the handle."""
    rt = simlib.runtime_lib()
    handle = 987654321
    for call in (lambda: rt.mwhip_shapes_compute(None, handle),
                 lambda: rt.mwhip_shapes_compute_async(None, handle),
                 lambda: rt.mwhip_set_step_shapes(None, handle, 1),
                 lambda: rt.mwhip_set_step_shapes(None, handle, 0)):
        assert call() == -3
        message = rt.mwhip_last_error().decode()
        assert "shape query %d is not one of this executor's" % handle in message, message
    nbytes = C.c_uint64(7)
    assert rt.mwhip_shapes_buffer(None, handle, 0, C.byref(nbytes)) is None
    assert str(handle) in rt.mwhip_last_error().decode()
    assert nbytes.value == 7
    rt.mwhip_shapes_destroy(None, handle)       # (harmless)


def test_a_descriptor_is_refused_without_an_executor(built):
    rt = simlib.runtime_lib()
    out = C.c_uint64(5)
    desc = simlib.ShapesDesc(4, 2, 8, 3, 0, 0)
    assert rt.mwhip_shapes_create(None, C.byref(desc), C.byref(out)) == -2
    assert rt.mwhip_shapes_create(None, None, C.byref(out)) == -2
    assert out.value == 5
    assert rt.mwhip_set_shape_kernel(None, None, 0) == -2


def test_python_surface():
    params = inspect.signature(simlib.Simulator.shape_query).parameters
    assert list(params) == ["self", "bundles", "shapes_per_bundle", "max_hits", "num_objects",
                            "world", "bundles_per_world", "count", "exclude", "plain"]
    assert [params[p].default for p in ("world", "bundles_per_world", "count", "exclude",
                                        "plain")] == [None, 0, None, None, False]
    for base in (simlib._Computed, simlib._Sourced, simlib._StepObject):
        assert issubclass(simlib.ShapeQuery, base)
    for member in ("worlds", "objects", "positions", "rotations", "scales", "excludes", "status",
                   "counts", "hits", "shape_is_ref", "num_points", "normals", "points",
                   "handle_source", "compute", "compute_async", "every_step", "close",
                   "buffer_ptr", "__enter__", "__exit__"):
        assert callable(getattr(simlib.ShapeQuery, member)), member
    assert inspect.signature(simlib.ShapeQuery.every_step).parameters["on"].default is True
    Q = simlib.ShapeQuery
    assert (Q.OK, Q.SKIPPED, Q.BAD_WORLD, Q.BAD_SHAPE, Q.UNSORTED, Q.UNSUPPORTED) == \
        (shape_ref.OK, shape_ref.SKIPPED, shape_ref.BAD_WORLD, shape_ref.BAD_SHAPE,
         shape_ref.UNSORTED, shape_ref.UNSUPPORTED) == (0, -1, -2, -3, -4, -5)
    assert list(inspect.signature(shape_ref.shape_ref).parameters) == [
        "worlds", "objects", "narrowphase", "shapes_per_bundle", "max_hits", "object_id",
        "position", "rotation", "scale", "world", "bundles_per_world", "count", "exclude",
        "num_objects", "unsorted"]


class _RefSim(simlib.Simulator):
    """A reference-backend simulator without a library."""

    def __init__(self):
        self.backend = "ref_cpu"
        self.handle = None
        self.num_worlds = 2
        self._shape_queries = []


def test_reference_backend_refuses():
    sim = _RefSim()
    try:
        sim.shape_query(2, 1, 8, 3)
    except RuntimeError as err:
        assert "HIP backend" in str(err)
    else:
        raise AssertionError("a shape query on the reference backend")
    assert sim._shape_queries == []


def test_cxx_surface_compiles_for_host_and_gfx950(built):
    """libshapes_conformance.so is linked from a host translation unit and a HIP
    one compiled for gfx950 that both name makeShapeQuery(), setStepShapes() and
    every member of MWHipShapeQuery; both saw the header's limits and codes."""
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libshapes_conformance.so"))
    for prefix in ("shapesconf_host", "shapesconf_hip"):
        traits = getattr(lib, prefix + "_traits")
        traits.restype = C.c_uint32
        assert traits() == 0b11111, prefix      # move-only
        got = getattr(lib, prefix + "_caps")
        got.restype = C.c_uint32
        assert got() == (4 << 16 | 13 << 8 | 1 << 4 | 5), prefix
        assert hasattr(lib, prefix + "_cycle"), prefix
    with open(os.path.join(HIP_BUILD_DIR, "libshapes_conformance.so"), "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"shapesconfTouch" in blob
    text = open(os.path.join(REPO_ROOT, "madrona_amd", "include", "madrona", "mw_gpu.hpp")).read()
    assert "class MWHipShapeQuery : public detail::ExecObject<detail::ShapeQueryKind>" in text
