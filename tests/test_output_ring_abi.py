"""CPU-only: the surface of the device-resident output rings exists at every
layer -- the C ABI (include/mwhip.h, added under ABI 9, exported by
libmadrona_hip.so), the C++ members of <madrona/mw_gpu.hpp> (compiled in a
conformance translation unit of their own, for the host and for gfx950:
tests/shims/ring_conformance*) and the Python wrapper (madrona_amd.simlib).  No
compute calls; the behaviour is tested on the GPU in
tests/test_output_ring_gpu.py."""
import ctypes as C
import inspect
import os
import re

from madrona_amd import simlib
from madrona_amd.simlib import HIP_BUILD_DIR, REPO_ROOT

RING_FUNCTIONS = ["mwhip_set_output_ring", "mwhip_output_ring_recorded"]


def _header():
    return open(os.path.join(REPO_ROOT, "include", "mwhip.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


def test_header_declares_the_two_functions():
    code = _code()
    assert re.search(r"\bint\s+mwhip_set_output_ring\s*\(\s*mwhip_exec\s*\*\s*\w+\s*,\s*"
                     r"const\s+void\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*,\s*"
                     r"uint64_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*\)", code)
    assert re.search(r"\bint\s+mwhip_output_ring_recorded\s*\(\s*mwhip_exec\s*\*\s*\w+\s*,\s*"
                     r"const\s+void\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*"
                     r"uint64_t\s*\*\s*\w+\s*\)", code)


def test_header_defines_the_three_macros():
    code = _code()
    assert re.search(r"#define\s+MWHIP_MAX_OUTPUT_RINGS\s+16\b", code)
    assert re.search(r"#define\s+MWHIP_RING_ON_STEP\s+0u\b", code)
    assert re.search(r"#define\s+MWHIP_RING_ON_RENDER\s+1u\b", code)
    assert (simlib.RING_ON_STEP, simlib.RING_ON_RENDER) == (0, 1)


def test_header_still_says_abi_9_and_names_the_additions():
    line = re.search(r"#define\s+MWHIP_ABI_VERSION\s+(\d+)u(.*)", _header())
    assert int(line.group(1)) == 9
    # the comment of the version says the two functions came under 9
    assert "mwhip_set_output_ring" in line.group(2)
    assert "mwhip_output_ring_recorded" in line.group(2)


def test_runtime_exports_the_two_functions(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    missing = [n for n in RING_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing


def test_refusals_come_before_the_executor_is_touched(built):
    """Arguments no executor could accept: every one is refused with a message
    (no GPU needed: the checks come first)."""
    rt = simlib.runtime_lib()
    src = C.c_void_p(0x1000)
    ring = C.c_void_p(0x2000)
    for args, word in (((None, None, ring, 4, 1, 0), b"source"),
                       ((None, src, ring, 4, 1, 2), b"when"),
                       ((None, src, ring, 4, 0, 0), b"slots"),
                       ((None, src, ring, 0, 1, 1), b"slots")):
        assert rt.mwhip_set_output_ring(*args) != 0, args
        assert word in rt.mwhip_last_error(), (args, rt.mwhip_last_error())
    out = C.c_uint64(7)
    assert rt.mwhip_output_ring_recorded(None, src, 0, C.byref(out)) != 0
    assert out.value == 7


def test_python_surface():
    assert callable(getattr(simlib.Simulator, "record"))
    params = inspect.signature(simlib.Simulator.record).parameters
    assert list(params) == ["self", "names", "steps", "on_render"]
    assert params["on_render"].default is False
    for member in ("slot", "close", "__getitem__"):
        assert callable(getattr(simlib.Trajectory, member)), member
    assert isinstance(inspect.getattr_static(simlib.Trajectory, "recorded"), property)
    # slot(k) is k % steps: no executor needed to say so
    traj = simlib.Trajectory.__new__(simlib.Trajectory)
    traj.steps = 5
    assert [traj.slot(k) for k in (0, 4, 5, 23)] == [0, 4, 0, 3]


def test_close_takes_the_trajectory_off_the_simulators_list():
    """The simulator holds open trajectories only (no executor needed to say
    so): a closed one's ring tensors die with the caller's last reference."""
    open_trajectories = []
    traj = simlib.Trajectory.__new__(simlib.Trajectory)
    traj._exec, traj._srcs, traj._open_in = 0, {}, open_trajectories
    other = simlib.Trajectory.__new__(simlib.Trajectory)
    open_trajectories += [other, traj]
    traj.close()
    assert open_trajectories == [other]
    traj.close()    # (twice is harmless)
    assert open_trajectories == [other]


def test_record_raises_on_the_reference_backend():
    class Ref(simlib.Simulator):
        def __init__(self):
            self.backend = "ref_cpu"
            self.handle = None

    try:
        Ref().record(["reward"], 4)
    except RuntimeError as err:
        assert "HIP backend" in str(err)
    else:
        raise AssertionError("Simulator.record() on the reference backend did not raise")


def test_cxx_surface_compiles_for_host_and_gfx950(built):
    """libring_conformance.so is linked from a host translation unit and a HIP
    one compiled for gfx950 that both name setOutputRing(), outputRingRecorded()
    and setInputRing(); both saw the header's three macros."""
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libring_conformance.so"))
    for prefix in ("ringconf_host", "ringconf_hip"):
        macros = getattr(lib, prefix + "_macros")
        macros.restype = C.c_uint32
        assert macros() == (16 << 16 | 1 << 8 | 0), prefix
        assert hasattr(lib, prefix + "_cycle"), prefix
    lib.ringconf_hip_kernel.restype = C.c_void_p
    # (the gfx950 code object is in the library: hipcc embeds it in this section)
    with open(os.path.join(HIP_BUILD_DIR, "libring_conformance.so"), "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"ringconfTouch" in blob
    # both translation units name the three members (the .inl they share does)
    inl = open(os.path.join(REPO_ROOT, "tests", "shims", "ring_conformance.inl")).read()
    for member in ("setOutputRing", "outputRingRecorded", "setInputRing"):
        assert "exec->%s(" % member in inl, member
