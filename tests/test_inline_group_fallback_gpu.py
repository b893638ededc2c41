"""What the runtime makes of a group named at compile time (madrona::SideBySide)
when a member is empty, tiny, wide, clashes with another or can append rows:
sort_stress' Config::groupCase (flags bits 8-10, sims/sort_stress/sim.cpp), each
case in lock step with its MADRONA_MWHIP_GROUP=0 run."""
import numpy as np
import pytest

from madrona_amd.simlib import Simulator, hip_lib_path

pytestmark = pytest.mark.gpu

STEPS = 12

IDLE, BLOB = "sortstress::groupIdleSystem", "sortstress::groupBlobSystem"
TAG, WIDE, QUAD = ("sortstress::groupChurnTagSystem", "sortstress::groupWide32System",
                   "sortstress::groupQuad64System")
WRITE, READ = "sortstress::siblingWriteSystem", "sortstress::siblingReadSystem"
APPENDER = "sortstress::groupAppenderSystem"

# case, worlds, the group launch expected (None: none), nodes with a launch of
# their own, in this order
CASES = [
    (1, 37, f"group[{IDLE} | {BLOB}]", []),             # a member without rows
    (2, 1, f"group[{TAG} | {BLOB}]", []),               # a member with ONE row
    (2, 37, f"group[{TAG} | {BLOB}]", []),
    (3, 1, f"group[{BLOB} | {WIDE} | {QUAD}]", []),     # 1, 32 and 64 lanes per row
    (3, 37, f"group[{BLOB} | {WIDE} | {QUAD}]", []),
    (4, 37, None, [WRITE, READ]),                       # clash on Quad: order kept
    (5, 37, None, [APPENDER, BLOB]),                    # a member can append rows
]


def _sim(monkeypatch, case, worlds, group):
    if group:
        monkeypatch.delenv("MADRONA_MWHIP_GROUP", raising=False)
    else:
        monkeypatch.setenv("MADRONA_MWHIP_GROUP", "0")
    return Simulator(hip_lib_path("sort_stress"), worlds, seed=7, flags=case << 8)


@pytest.mark.parametrize("case,worlds,group,own", CASES)
def test_group_case(built, monkeypatch, case, worlds, group, own):
    with _sim(monkeypatch, case, worlds, True) as a, \
            _sim(monkeypatch, case, worlds, False) as b:
        for step in range(1, STEPS + 1):
            a.step(1)
            b.step(1)
            if step % 3 == 0:
                assert a.read_tensor("churn").tobytes() == b.read_tensor("churn").tobytes(), step
                da, db = a.dump_all(), b.dump_all()
                assert da.keys() == db.keys()
                for col in da:
                    for xa, xb in zip(da[col], db[col]):
                        assert np.asarray(xa).tobytes() == np.asarray(xb).tobytes(), (step, col)
        names = [k["name"] for k in a.profile(2)]
        apart = [k["name"] for k in b.profile(2)]
    print(names)
    ours = [n for n in names if "sortstress::group" in n or "sortstress::sibling" in n]
    if group is not None:
        assert ours == [group], names
    else:
        assert ours == own, names
    # (every node its own launch: the members in registration order)
    assert [n for n in apart if n.startswith("group[")] == [], apart
