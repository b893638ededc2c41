"""CPU-only: the surface of executor snapshots exists at every layer -- the C ABI
(include/mwhip.h, ABI 9, exported by libmadrona_hip.so), the C++ classes of
<madrona/mw_gpu.hpp> (compiled in a conformance translation unit of their own,
for the host and for gfx950: tests/shims/snapshot_conformance*) and the Python
wrapper (madrona_amd.simlib).  No compute calls; the behaviour is tested on the
GPU in tests/test_snapshot_gpu.py."""
import ctypes as C
import inspect
import os
import re

from madrona_amd import simlib
from madrona_amd.simlib import HIP_BUILD_DIR, REPO_ROOT

SNAPSHOT_FUNCTIONS = ["mwhip_snapshot_create", "mwhip_snapshot_destroy",
                      "mwhip_snapshot_save", "mwhip_snapshot_restore",
                      "mwhip_snapshot_save_async", "mwhip_snapshot_restore_async",
                      "mwhip_snapshot_bytes"]


def _header():
    return open(os.path.join(REPO_ROOT, "include", "mwhip.h")).read()


def test_header_says_abi_9():
    version = int(re.search(r"#define\s+MWHIP_ABI_VERSION\s+(\d+)u", _header()).group(1))
    assert version == 9


def test_header_declares_the_seven_functions():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in SNAPSHOT_FUNCTIONS:
        assert re.search(r"\b%s\s*\(\s*mwhip_exec\s*\*" % name, code), name


def test_runtime_exports_the_seven_functions(built):
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    missing = [n for n in SNAPSHOT_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing


def test_unknown_handles_are_refused_without_an_executor_state(built):
    """A handle no executor made: every entry point says so instead of touching
    anything (no GPU needed: the lookup comes first)."""
    rt = simlib.runtime_lib()
    for name in ("mwhip_snapshot_save", "mwhip_snapshot_restore",
                 "mwhip_snapshot_save_async", "mwhip_snapshot_restore_async"):
        assert getattr(rt, name)(None, 12345) != 0, name
        assert b"snapshot 12345" in rt.mwhip_last_error(), name
    assert rt.mwhip_snapshot_bytes(None, 12345) == 0
    rt.mwhip_snapshot_destroy(None, 12345)


def test_python_surface():
    assert callable(getattr(simlib.Simulator, "snapshot"))
    for member in ("save", "restore", "save_async", "restore_async", "close"):
        assert callable(getattr(simlib.Snapshot, member)), member
    assert isinstance(inspect.getattr_static(simlib.Snapshot, "nbytes"), property)


def test_snapshot_raises_on_the_reference_backend():
    class Ref(simlib.Simulator):
        def __init__(self):
            self.backend = "ref_cpu"
            self.handle = None

    try:
        Ref().snapshot()
    except RuntimeError as err:
        assert "HIP backend" in str(err)
    else:
        raise AssertionError("Simulator.snapshot() on the reference backend did not raise")


def test_cxx_surface_compiles_for_host_and_gfx950(built):
    """libsnapshot_conformance.so is linked from a host translation unit and a
    HIP one compiled for gfx950 that both name makeSnapshot() and every member
    of MWHipSnapshot; both report the class as move-only."""
    C.CDLL(os.path.join(HIP_BUILD_DIR, "libmadrona_hip.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(HIP_BUILD_DIR, "libsnapshot_conformance.so"))
    for prefix in ("snapconf_host", "snapconf_hip"):
        traits = getattr(lib, prefix + "_traits")
        traits.restype = C.c_uint32
        assert traits() == 0b11111, prefix
        assert hasattr(lib, prefix + "_cycle"), prefix
    lib.snapconf_hip_kernel.restype = C.c_void_p
    # (the gfx950 code object is in the library: hipcc embeds it in this section)
    with open(os.path.join(HIP_BUILD_DIR, "libsnapshot_conformance.so"), "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"snapconfTouch" in blob
