"""CPU-only: the surface of ray queries exists at every layer -- the C ABI
(include/mwhip.h, added under ABI 9, exported by libmadrona_hip.so), the kernel's
place in the physics headers, and the Python wrapper (madrona_amd.simlib)."""
import ctypes as C
import inspect
import os
import re
import subprocess

from madrona_amd import ray_ref, simlib
from madrona_amd.simlib import HIP_BUILD_DIR, REPO_ROOT

RAY_FUNCTIONS = ["mwhip_set_ray_kernel", "mwhip_rays_create", "mwhip_rays_destroy",
                 "mwhip_rays_compute", "mwhip_rays_compute_async", "mwhip_rays_buffer",
                 "mwhip_set_step_rays"]


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
            r"\bint\s+mwhip_set_ray_kernel\s*\(\s*%s\s*,\s*const\s+void\s*\*\s*\w+\s*\)" % E,
            r"\bint\s+mwhip_rays_create\s*\(\s*%s\s*,\s*const\s+mwhip_rays_desc\s*\*\s*\w+"
            r"\s*,\s*uint64_t\s*\*\s*\w+\s*\)" % E,
            r"\bvoid\s+mwhip_rays_destroy\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_rays_compute\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_rays_compute_async\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bvoid\s*\*\s*mwhip_rays_buffer\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,"
            r"\s*uint64_t\s*\*\s*\w+\s*\)" % (E, U64, U32),
            r"\bint\s+mwhip_set_step_rays\s*\(\s*%s\s*,\s*%s\s*,\s*int\s+\w+\s*\)" % (E, U64)):
        assert re.search(pattern, code), pattern
    assert re.search(r"#define\s+MWHIP_MAX_STEP_RAYS\s+4\b", code)
    for name, value in (("HIT", "1"), ("MISS", "0"), ("SKIPPED", r"\(-1\)"),
                        ("BAD_WORLD", r"\(-2\)"), ("BAD_RAY", r"\(-3\)")):
        assert re.search(r"#define\s+MWHIP_RAYS_%s\s+%s\s" % (name, value), code), name
    assert _struct(code, "mwhip_ray_source") == ["src", "record_bytes", "first_byte"]
    assert _struct(code, "mwhip_rays_desc") == ["num_fans", "rays_per_fan", "fans_per_world",
                                                "pad_", "world", "count", "origin"]
    assert _struct(code, "mwhip_ray_args") == ["num_plans", "pad_", "items", "plans"]
    assert "groups_per_fan" in _struct(code, "mwhip_ray_plan")


def test_header_still_says_abi_9_and_names_the_additions():
    line = re.search(r"#define\s+MWHIP_ABI_VERSION\s+(\d+u)(.*)", _header())
    assert line.group(1) == "9u"
    for word in ("mwhip_rays_", "mwhip_set_step_rays", "mwhip_set_ray_kernel", "mwhip_rays_desc"):
        assert word in line.group(2), word


def test_header_says_what_a_ray_sees():
    text = " ".join(_header().replace(" * ", " ").split())
    section = text[text.index("Ray queries (added under ABI 9)"):]
    section = section[: section.index("#define MWHIP_MAX_STEP_RAYS")]
    for phrase in ("LAST BROADPHASE PASS left it", "spheres are transparent",
                   "this simulator registered no ray kernel", "-3 for an unknown handle",
                   "-10 for buffers"):
        assert phrase in section, phrase
    bvh = open(os.path.join(REPO_ROOT, "madrona_amd", "include", "madrona", "phys_impl",
                            "ray_query.inl")).read()
    assert "last broadphase pass" in bvh and "spheres are transparent" in bvh


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "rays_abi_check.c"
    src.write_text(
        '#include "mwhip.h"\n'
        "int main(void)\n{\n"
        "    uint64_t rays = 0, bytes = 0;\n"
        "    mwhip_rays_desc desc = { 2, 30, 0, 0, { 0, 0, 0 }, { 0, 0, 0 }, { &bytes, 12, 0 } };\n"
        "    mwhip_ray_args args = { 0, 0, { 0 }, { 0 } };\n"
        "    mwhip_ray_plan plan = { 0 };\n"
        "    int rc = mwhip_rays_create(0, &desc, &rays) | mwhip_set_ray_kernel(0, 0);\n"
        "    rc |= mwhip_rays_compute(0, rays) | mwhip_rays_compute_async(0, rays);\n"
        "    rc |= mwhip_set_step_rays(0, rays, MWHIP_MAX_STEP_RAYS != 0);\n"
        "    rc |= mwhip_rays_buffer(0, rays, MWHIP_RAYS_BUF_STATUS, &bytes) != 0;\n"
        "    rc |= MWHIP_RAYS_HIT + MWHIP_RAYS_MISS + MWHIP_RAYS_SKIPPED + MWHIP_RAYS_BAD_WORLD\n"
        "        + MWHIP_RAYS_BAD_RAY + (int)MWHIP_RAYS_NUM_BUFS + (int)args.num_plans\n"
        "        + (int)plan.num_fans;\n"
        "    mwhip_rays_destroy(0, rays);\n"
        "    return rc + (int)sizeof(desc) - 64 + (int)sizeof(args) - 56\n"
        "        + (int)sizeof(plan) - 112;\n}\n")
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I",
                          os.path.join(REPO_ROOT, "include"), str(src), "-c", "-o",
                          str(tmp_path / "rays_abi_check.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_struct_sizes_agree_with_python():
    assert C.sizeof(simlib.RaySource) == 16 and C.sizeof(simlib.RaysDesc) == 64
    assert [f[0] for f in simlib.RaysDesc._fields_] == [
        "num_fans", "rays_per_fan", "fans_per_world", "pad_", "world", "count", "origin"]
    assert [f[0] for f in simlib.RaySource._fields_] == ["src", "record_bytes", "first_byte"]


def test_runtime_exports_them(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    missing = [n for n in RAY_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing


def test_every_simulator_with_a_broadphase_carries_the_kernel(built):
    """The kernel is compiled into the simulator's code object, for gfx950."""
    for sim, has in (("broadphase_only", True), ("escape_room_phys", True), ("hideseek", True),
                     ("cartpole", False)):
        with open(simlib.hip_lib_path(sim), "rb") as f:
            blob = f.read()
        assert (b"rayQueryKernel" in blob) == has, sim
        assert b"gfx950" in blob


def test_an_unknown_handle_is_refused_with_a_null_executor(built):
    """The lookup comes first: no executor (and no GPU) needed, and the message
    names the handle."""
    rt = simlib.runtime_lib()
    handle = 987654321
    for call in (lambda: rt.mwhip_rays_compute(None, handle),
                 lambda: rt.mwhip_rays_compute_async(None, handle),
                 lambda: rt.mwhip_set_step_rays(None, handle, 1),
                 lambda: rt.mwhip_set_step_rays(None, handle, 0)):
        assert call() == -3
        message = rt.mwhip_last_error().decode()
        assert "ray query %d is not one of this executor's" % handle in message, message
    nbytes = C.c_uint64(7)
    assert rt.mwhip_rays_buffer(None, handle, 0, C.byref(nbytes)) is None
    assert str(handle) in rt.mwhip_last_error().decode()
    assert nbytes.value == 7
    rt.mwhip_rays_destroy(None, handle)      # (harmless)


def test_a_bad_descriptor_is_refused_without_an_executor(built):
    rt = simlib.runtime_lib()
    out = C.c_uint64(5)
    desc = simlib.RaysDesc(2, 30, 0, 0)
    assert rt.mwhip_rays_create(None, C.byref(desc), C.byref(out)) == -2
    assert rt.mwhip_rays_create(None, None, C.byref(out)) == -2
    assert out.value == 5
    assert rt.mwhip_set_ray_kernel(None, None) == -2


def test_python_surface():
    params = inspect.signature(simlib.Simulator.ray_query).parameters
    assert list(params) == ["self", "fans", "rays_per_fan", "world", "origin", "fans_per_world",
                            "count"]
    assert [params[p].default for p in ("world", "origin", "fans_per_world", "count")] == [
        None, None, 0, None]
    assert issubclass(simlib.RayQuery, simlib._ExecObject)
    for member in ("worlds", "origins", "directions", "t_max", "hit_t", "hits", "normals",
                   "status", "handle_source", "compute", "compute_async", "every_step", "close",
                   "buffer_ptr", "__enter__", "__exit__"):
        assert callable(getattr(simlib.RayQuery, member)), member
    assert inspect.signature(simlib.RayQuery.every_step).parameters["on"].default is True
    assert (simlib.RayQuery.HIT, simlib.RayQuery.MISS, simlib.RayQuery.SKIPPED,
            simlib.RayQuery.BAD_WORLD, simlib.RayQuery.BAD_RAY) == \
        (ray_ref.HIT, ray_ref.MISS, ray_ref.SKIPPED, ray_ref.BAD_WORLD, ray_ref.BAD_RAY)
    assert list(inspect.signature(ray_ref.ray_ref).parameters) == [
        "trace", "num_worlds", "fans", "rays_per_fan", "directions", "t_max", "origin", "world",
        "fans_per_world", "count"]


class _RefSim(simlib.Simulator):
    """A reference-backend simulator without a library."""

    def __init__(self):
        self.backend = "ref_cpu"
        self.handle = None
        self.num_worlds = 2
        self._ray_queries = []


def test_reference_backend_refuses():
    sim = _RefSim()
    try:
        sim.ray_query(2, 30)
    except RuntimeError as err:
        assert "HIP backend" in str(err)
    else:
        raise AssertionError("a ray query on the reference backend")
    assert sim._ray_queries == []


def test_cxx_surface_compiles_for_host_and_gfx950(built):
    """librays_conformance.so is linked from a host translation unit and a HIP
    one compiled for gfx950 that both name makeRayQuery(), setStepRays() and
    every member of MWHipRayQuery; both saw the header's limits and codes."""
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "librays_conformance.so"))
    for prefix in ("raysconf_host", "raysconf_hip"):
        traits = getattr(lib, prefix + "_traits")
        traits.restype = C.c_uint32
        assert traits() == 0b11111, prefix      # move-only
        got = getattr(lib, prefix + "_caps")
        got.restype = C.c_uint32
        assert got() == (4 << 16 | 8 << 8 | 4), prefix
        assert hasattr(lib, prefix + "_cycle"), prefix
    with open(os.path.join(HIP_BUILD_DIR, "librays_conformance.so"), "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"raysconfTouch" in blob
    inl = open(os.path.join(REPO_ROOT, "tests", "shims", "rays_conformance.inl")).read()
    for member in ("exec->makeRayQuery(", "exec->setStepRays(", ".compute()", ".computeAsync()",
                   ".worldsTensor()", ".originsTensor()", ".directionsTensor()", ".tMaxTensor()",
                   ".hitTTensor()", ".hitsTensor()", ".normalsTensor()", ".statusTensor()",
                   ".handleSource()", ".numFans()", ".numRays()", "MWHIP_ABI_VERSION == 9u"):
        assert member in inl, member
    text = open(os.path.join(REPO_ROOT, "madrona_amd", "include", "madrona", "mw_gpu.hpp")).read()
    assert "class MWHipRayQuery : public detail::ExecObject<detail::RayQueryKind>" in text
