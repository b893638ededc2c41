"""CPU-only: the surface of contact queries exists at every layer -- the C ABI
(include/mwhip.h, added under ABI 9, exported by libmadrona_hip.so), the kernel's
place in the physics headers and in the simulators' code objects, the C++
wrapper (madrona/mw_gpu.hpp) and the Python one (madrona_amd.simlib)."""
import ctypes as C
import inspect
import os
import re
import subprocess

from madrona_amd import contact_ref, simlib
from madrona_amd.simlib import HIP_BUILD_DIR, REPO_ROOT

CONTACT_FUNCTIONS = ["mwhip_set_contact_kernel", "mwhip_contacts_create",
                     "mwhip_contacts_destroy", "mwhip_contacts_compute",
                     "mwhip_contacts_compute_async", "mwhip_contacts_buffer",
                     "mwhip_set_step_contacts"]


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
            r"\bint\s+mwhip_set_contact_kernel\s*\(\s*%s\s*,\s*const\s+void\s*\*\s*\w+\s*,"
            r"\s*%s\s*\)" % (E, U32),
            r"\bint\s+mwhip_contacts_create\s*\(\s*%s\s*,\s*const\s+mwhip_contacts_desc\s*\*"
            r"\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)" % E,
            r"\bvoid\s+mwhip_contacts_destroy\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_contacts_compute\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bint\s+mwhip_contacts_compute_async\s*\(\s*%s\s*,\s*%s\s*\)" % (E, U64),
            r"\bvoid\s*\*\s*mwhip_contacts_buffer\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,"
            r"\s*uint64_t\s*\*\s*\w+\s*\)" % (E, U64, U32),
            r"\bint\s+mwhip_set_step_contacts\s*\(\s*%s\s*,\s*%s\s*,\s*int\s+\w+\s*\)" % (E, U64)):
        assert re.search(pattern, code), pattern
    assert re.search(r"#define\s+MWHIP_MAX_STEP_CONTACTS\s+4\b", code)
    assert re.search(r"#define\s+MWHIP_CONTACTS_CURRENT_POSES\s+1u\b", code)
    assert re.search(r"#define\s+MWHIP_CONTACTS_PLAIN\s+2u\b", code)
    assert re.search(r"#define\s+MWHIP_CONTACT_CAP_SOLVER_POSES\s+1u\b", code)
    for name, value in (("OK", "0"), ("SKIPPED", r"\(-1\)"), ("UNSORTED", r"\(-2\)"),
                        ("UNSUPPORTED", r"\(-3\)")):
        assert re.search(r"#define\s+MWHIP_CONTACTS_%s\s+%s\s" % (name, value), code), name
    for k, name in enumerate(("SELECT", "STATUS", "COUNT", "PAIRS", "NUM_POINTS", "NORMAL",
                              "POINTS")):
        assert re.search(r"#define\s+MWHIP_CONTACTS_BUF_%s\s+%du\b" % (name, k), code), name
    assert re.search(r"#define\s+MWHIP_CONTACTS_NUM_BUFS\s+7u\b", code)
    assert _struct(code, "mwhip_contacts_desc") == [
        "max_contacts", "flags", "own_select", "pad_", "select"]
    assert _struct(code, "mwhip_contact_args") == ["num_plans", "pad_", "items", "plans"]
    plan = _struct(code, "mwhip_contact_plan")
    for field in ("state", "select_src", "status", "count", "pairs", "num_points", "normal",
                  "points", "max_contacts", "flags", "num_worlds"):
        assert field in plan, field


def test_header_still_says_abi_9_and_names_the_additions():
    line = re.search(r"#define\s+MWHIP_ABI_VERSION\s+(\d+u)(.*)", _header())
    assert line.group(1) == "9u"
    for word in ("mwhip_contacts_", "mwhip_set_step_contacts", "mwhip_set_contact_kernel",
                 "mwhip_contacts_desc", "mwhip_contact_args"):
        assert word in line.group(2), word
    assert "no struct a simulator library is compiled against changed" in line.group(2)


def test_header_says_what_a_contact_is():
    text = " ".join(_header().replace(" * ", " ").split())
    section = text[text.index("Contact queries (added under ABI 9)"):]
    section = section[: section.index("#define MWHIP_MAX_STEP_CONTACTS")]
    for phrase in ("LOWER ENTITY ID", "NOT capped by K", "SOLVER POSES", "exactly (0, 0, 0, 0)",
                   "this simulator has no solver poses", "-3 for an unknown handle",
                   "-10 for buffers", "No BVH is involved", "No sticky error flag",
                   "ORDER: ascending (k_lo, k_hi, aPrim", "b_num_prims + bPrim)",
                   "snapshots do not save them"):
        assert phrase in section, phrase
    inl = open(os.path.join(REPO_ROOT, "madrona_amd", "include", "madrona", "phys_impl",
                            "contact_query.inl")).read()
    for name in ("contactQueryKernel", "collidePairLane(", "hullHullWave(", "collidePairStored(",
                 "WorldBodies bodies", "setupPair("):
        assert name in inl, name
    phys = open(os.path.join(REPO_ROOT, "madrona_amd", "include", "madrona", "physics.inl")).read()
    assert phys.index("#include <madrona/phys_impl/box_query.inl>") < \
        phys.index("#include <madrona/phys_impl/contact_query.inl>")
    assert "mwhip_set_contact_kernel(builder.exec()" in phys


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "contacts_abi_check.c"
    src.write_text(
        '#include "mwhip.h"\n'
        "int main(void)\n{\n"
        "    uint64_t contacts = 0, bytes = 0;\n"
        "    mwhip_contacts_desc desc = { 32, MWHIP_CONTACTS_CURRENT_POSES | MWHIP_CONTACTS_PLAIN,\n"
        "                                 0, 0, { &bytes, 4, 0 } };\n"
        "    mwhip_contact_args args = { 0, 0, { 0 }, { 0 } };\n"
        "    mwhip_contact_plan plan = { 0 };\n"
        "    int rc = mwhip_contacts_create(0, &desc, &contacts)\n"
        "        | mwhip_set_contact_kernel(0, 0, MWHIP_CONTACT_CAP_SOLVER_POSES);\n"
        "    rc |= mwhip_contacts_compute(0, contacts) | mwhip_contacts_compute_async(0, contacts);\n"
        "    rc |= mwhip_set_step_contacts(0, contacts, MWHIP_MAX_STEP_CONTACTS != 0);\n"
        "    rc |= mwhip_contacts_buffer(0, contacts, MWHIP_CONTACTS_BUF_PAIRS, &bytes) != 0;\n"
        "    rc |= MWHIP_CONTACTS_OK + MWHIP_CONTACTS_SKIPPED + MWHIP_CONTACTS_UNSORTED\n"
        "        + MWHIP_CONTACTS_UNSUPPORTED + (int)MWHIP_CONTACTS_NUM_BUFS\n"
        "        + (int)MWHIP_CONTACTS_BUF_SELECT + (int)MWHIP_CONTACTS_BUF_STATUS\n"
        "        + (int)MWHIP_CONTACTS_BUF_COUNT + (int)MWHIP_CONTACTS_BUF_NUM_POINTS\n"
        "        + (int)MWHIP_CONTACTS_BUF_NORMAL + (int)MWHIP_CONTACTS_BUF_POINTS\n"
        "        + (int)args.num_plans + (int)plan.num_worlds;\n"
        "    mwhip_contacts_destroy(0, contacts);\n"
        "    return rc + (int)sizeof(desc) - 32 + (int)sizeof(args) - 56\n"
        "        + (int)sizeof(plan) - 80;\n}\n")
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I",
                          os.path.join(REPO_ROOT, "include"), str(src), "-c", "-o",
                          str(tmp_path / "contacts_abi_check.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_struct_sizes_agree_with_python():
    assert C.sizeof(simlib.ContactsDesc) == 32
    assert [f[0] for f in simlib.ContactsDesc._fields_] == [
        "max_contacts", "flags", "own_select", "pad_", "select"]


def test_runtime_exports_them(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    missing = [n for n in CONTACT_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing


def test_every_simulator_with_a_rigid_body_step_carries_the_kernel(built):
    """The kernel is compiled into the simulator's code object, for gfx950.
    (broadphase_only includes the physics headers and so carries the code, but
    sets up no step and registers nothing: tests/test_contact_query_gpu.py.)"""
    for sim, has in (("contact_probe", True), ("escape_room_phys", True), ("hideseek", True),
                     ("ball_pit", True), ("tgs_drop", True), ("cartpole", False)):
        with open(simlib.hip_lib_path(sim), "rb") as f:
            blob = f.read()
        assert (b"contactQueryKernel" in blob) == has, sim
        assert b"gfx950" in blob


def test_an_unknown_handle_is_refused_with_a_null_executor(built):
    """The lookup comes first: no executor (and no GPU) needed, and the message
    names the handle."""
    rt = simlib.runtime_lib()
    handle = 987654321
    for call in (lambda: rt.mwhip_contacts_compute(None, handle),
                 lambda: rt.mwhip_contacts_compute_async(None, handle),
                 lambda: rt.mwhip_set_step_contacts(None, handle, 1),
                 lambda: rt.mwhip_set_step_contacts(None, handle, 0)):
        assert call() == -3
        message = rt.mwhip_last_error().decode()
        assert "contact query %d is not one of this executor's" % handle in message, message
    nbytes = C.c_uint64(7)
    assert rt.mwhip_contacts_buffer(None, handle, 0, C.byref(nbytes)) is None
    assert str(handle) in rt.mwhip_last_error().decode()
    assert nbytes.value == 7
    rt.mwhip_contacts_destroy(None, handle)     # (harmless)


def test_a_descriptor_is_refused_without_an_executor(built):
    rt = simlib.runtime_lib()
    out = C.c_uint64(5)
    desc = simlib.ContactsDesc(8, 0, 0, 0)
    assert rt.mwhip_contacts_create(None, C.byref(desc), C.byref(out)) == -2
    assert rt.mwhip_contacts_create(None, None, C.byref(out)) == -2
    assert out.value == 5
    assert rt.mwhip_set_contact_kernel(None, None, 0) == -2


def test_python_surface():
    params = inspect.signature(simlib.Simulator.contact_query).parameters
    assert list(params) == ["self", "max_contacts", "select", "poses", "plain"]
    assert [params[p].default for p in ("select", "poses", "plain")] == [None, "solver", False]
    assert issubclass(simlib.ContactQuery, simlib._Computed)
    assert issubclass(simlib.ContactQuery, simlib._StepObject)
    for member in ("status", "counts", "pairs", "num_points", "normals", "points", "selects",
                   "handle_source", "compute", "compute_async", "every_step", "close",
                   "buffer_ptr", "__enter__", "__exit__"):
        assert callable(getattr(simlib.ContactQuery, member)), member
    assert inspect.signature(simlib.ContactQuery.every_step).parameters["on"].default is True
    assert (simlib.ContactQuery.OK, simlib.ContactQuery.SKIPPED, simlib.ContactQuery.UNSORTED,
            simlib.ContactQuery.UNSUPPORTED) == \
        (contact_ref.OK, contact_ref.SKIPPED, contact_ref.UNSORTED, contact_ref.UNSUPPORTED)
    assert list(inspect.signature(contact_ref.contact_ref).parameters) == [
        "worlds", "objects", "narrowphase", "max_contacts", "select", "poses", "unsorted"]


class _RefSim(simlib.Simulator):
    """A reference-backend simulator without a library."""

    def __init__(self):
        self.backend = "ref_cpu"
        self.handle = None
        self.num_worlds = 2
        self._contact_queries = []


def test_reference_backend_refuses():
    sim = _RefSim()
    try:
        sim.contact_query(8)
    except RuntimeError as err:
        assert "HIP backend" in str(err)
    else:
        raise AssertionError("a contact query on the reference backend")
    assert sim._contact_queries == []


def test_cxx_surface_compiles_for_host_and_gfx950(built):
    """libcontacts_conformance.so is linked from a host translation unit and a
    HIP one compiled for gfx950 that both name makeContactQuery(),
    setStepContacts() and every member of MWHipContactQuery; both saw the
    header's limits and codes."""
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libcontacts_conformance.so"))
    for prefix in ("contactsconf_host", "contactsconf_hip"):
        traits = getattr(lib, prefix + "_traits")
        traits.restype = C.c_uint32
        assert traits() == 0b11111, prefix      # move-only
        got = getattr(lib, prefix + "_caps")
        got.restype = C.c_uint32
        assert got() == (4 << 16 | 7 << 8 | 3 << 4 | 3), prefix
        assert hasattr(lib, prefix + "_cycle"), prefix
    with open(os.path.join(HIP_BUILD_DIR, "libcontacts_conformance.so"), "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"contactsconfTouch" in blob
    text = open(os.path.join(REPO_ROOT, "madrona_amd", "include", "madrona", "mw_gpu.hpp")).read()
    assert "class MWHipContactQuery : public detail::ExecObject<detail::ContactQueryKind>" in text
