"""Box queries (mwhip_boxes_*, Simulator.box_query) on the device.
The yardsticks are not the code under test: Prober.Probe32 of broadphase_only's
plan mode (in lock step with the reference, test_bvh_edges_gpu.py), the float32
brute force over axis-aligned cubes (pos -/+ scale * 0.5, strict comparisons;
tests/test_bvh_edges_cpu.py shows the reference satisfies it), the restated
build's traversal order (bvh_edges_utils.restated_build), and the packed mapping
-- plain findEntitiesWithinAABB, a box per lane -- for the cooperative one."""
import numpy as np
import pytest

import bvh_edges_utils as U
from madrona_amd.simlib import RING_ON_STEP, Simulator, hip_lib_path, runtime_lib

pytestmark = pytest.mark.gpu

OK, SKIPPED, BAD_WORLD, BAD_BOX = 0, -1, -2, -3
W = 29          # the 28-entry leaf table and one more
K = 160
COLUMNS = ("Box.Entity", "Box.Position", "Box.Scale", "Box.Velocity", "Box.LeafID",
           "Pillar.Entity", "Pillar.LeafID", "Sensor.Position", "Sensor.RayFan",
           "Sensor.RayFanPlain", "Prober.Probe32")


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _plan(layout, monkeypatch, worlds=W):
    # (130 coincident boxes make 8385 candidate pairs)
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CANDIDATES_PER_WORLD", "2048")
    return Simulator(hip_lib_path("broadphase_only"), worlds, seed=5,
                     flags=U.plan_flags(layout))


def _dump(sim, names=COLUMNS):
    listed = [c[0] for c in sim.columns]
    return {name: sim.dump_column(listed.index(name), 256) for name in names}


def _set(tensor, values):
    """Writes a query's tensor and WAITS (the executor's stream is non-blocking:
    the ordering is the caller's)."""
    torch = _torch()
    tensor.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(tensor.device))
    torch.cuda.synchronize()


def _out(q):
    """(status int32 [B], count int32 [B], hits int32 [B, K, 2])"""
    _torch().cuda.synchronize()
    return (q.status().cpu().numpy(), q.counts().cpu().numpy(), q.hits().cpu().numpy())


def _same(a, b, what):
    for x, y, name in zip(a, b, ("status", "count", "hits")):
        bad = np.argwhere(x != y)
        assert bad.size == 0, (what, name, bad[:4])


def _probe_corners(dump):
    """(lo, hi) float32 [W, 4, 3]: the corners probeWorld computes
    (centres[k] -/+ PROBE_HALF[k]), from the dump, in float32"""
    f = np.float32
    bodies = U.world_bodies(dump)
    sensors = U.world_sensors(dump)
    lo = np.zeros((len(bodies), 4, 3), f)
    hi = np.zeros((len(bodies), 4, 3), f)
    for w, (body, (s_pos, _, _)) in enumerate(zip(bodies, sensors)):
        first_box = body["pos"][0] if body["dynamic"].any() else np.zeros(3, f)
        for k, centre in enumerate((first_box, s_pos[0], s_pos[-1], s_pos[0])):
            lo[w, k] = centre.astype(f) - f(U.PROBE_HALF[k])
            hi[w, k] = centre.astype(f) + f(U.PROBE_HALF[k])
    return lo, hi, bodies


def _absolute(sim, per_world, max_hits=K, **kwargs):
    """a query of W bundles of per_world boxes with absolute corners"""
    q = sim.box_query(sim.num_worlds, per_world, max_hits, **kwargs)
    _set(q.worlds(), np.arange(sim.num_worlds, dtype=np.int32))
    return q


# ---- 1 + 4. the simulator's own probes; K ------------------------------------------------
@pytest.mark.parametrize("layout", ["drift", "coincident"])
def test_first_dynamic_hit_is_the_simulators_probe_and_k_cuts_prefixes(built, monkeypatch,
                                                                       layout):
    """Plan mode, 29 worlds, 9 steps, a rebuild every 4: per probe box the first
    hit that is a Box is Prober.Probe32 (-1 where none is); the world without a
    leaf has count 0.  K = 1, 3 and 33 give the prefixes of K = 160's lists and
    the same counts -- the world of 130 coincident leaves included, whose largest
    count is all 130 of them."""
    with _plan(layout, monkeypatch) as s:
        s.step(1)
        q = _absolute(s, 4)
        small = {k: _absolute(s, 4, k) for k in (1, 3, 33)}
        assert not q.status().cpu().numpy().any() and not q.counts().cpu().numpy().any()
        assert (q.hits().cpu().numpy() == -1).all()        # at creation
        found = 0
        for step in range(1, 10):
            if step > 1:
                s.step(1)
            dump = _dump(s)
            lo, hi, bodies = _probe_corners(dump)
            p32 = dump["Prober.Probe32"][0].view(np.int32).reshape(-1, 4)
            for query in (q, *small.values()):
                _set(query.lo(), lo.reshape(-1, 3))
                _set(query.hi(), hi.reshape(-1, 3))
            status, count, hits = _out(q.compute())
            assert not status.any()
            hits = hits.reshape(W, 4, K, 2)
            count = count.reshape(W, 4)
            for w, body in enumerate(bodies):
                box_ids = body["id"][body["dynamic"]]
                for k in range(4):
                    ids = hits[w, k, :min(count[w, k], K), 1]
                    assert (hits[w, k, count[w, k]:] == -1).all()
                    dyn = ids[np.isin(ids, box_ids)]
                    first = int(dyn[0]) if len(dyn) else -1
                    assert first == p32[w, k], (layout, step, w, k, first, p32[w, k])
                    found += first >= 0
                if len(body["id"]) == 0:
                    assert not count[w].any()
            assert any(len(b["id"]) == 0 for b in bodies)
            for k, query in small.items():
                s_k, c_k, h_k = _out(query.compute())
                assert np.array_equal(c_k, count.ravel()) and not s_k.any()
                assert np.array_equal(h_k.reshape(W, 4, k, 2), hits[:, :, :k]), (layout, step, k)
            if layout == "coincident":
                # (the world of 130 leaves: 126 coincident boxes and 4 pillars, all
                # of them inside the all-containing probe box)
                assert count.max() == 130
        assert found > 9 * W


# ---- 2. whole lists against brute force --------------------------------------------------
def _random_boxes(seed, worlds, per_world):
    rng = np.random.default_rng(seed)
    centre = np.stack([rng.uniform(-5, 5, (worlds, per_world)),
                       rng.uniform(-5, 5, (worlds, per_world)),
                       rng.uniform(0, 4, (worlds, per_world))], -1).astype(np.float32)
    half = np.exp(rng.uniform(np.log(0.05), np.log(6.0), (worlds, per_world, 3))).astype(np.float32)
    return (centre - half).astype(np.float32), (centre + half).astype(np.float32)


# (checked on the reference backend's dumps of both layouts, 9 steps: the
# exclusion rule leaves out no box of this seed; seed 7, for one, loses one)
LIST_SEED = 1


@pytest.mark.parametrize("layout", ["drift", "coincident"])
def test_whole_lists_against_brute_force(built, monkeypatch, layout):
    """8 boxes per world from a fixed seed: the set of hit ids is the brute-force
    set over boxes and pillars, count its size, no id twice, every hit a live
    generation.  No box of the seed lies within 1e-5 (relative) of a body face
    on an axis that decides the overlap: asserted, not skipped.  Right after a
    rebuild, in worlds of more than 32 bodies, hits come in increasing rank of
    the restated traversal order; some rank is >= 32 and some count above 32."""
    G = 8
    q_lo, q_hi = _random_boxes(LIST_SEED, W, G)
    with _plan(layout, monkeypatch) as s:
        q = _absolute(s, G)
        _set(q.lo(), q_lo.reshape(-1, 3))
        _set(q.hi(), q_hi.reshape(-1, 3))
        late, big = 0, 0
        for step in range(1, 10):
            s.step(1)
            dump = _dump(s)
            bodies = U.world_bodies(dump)
            gens = {}
            for table in ("Box", "Pillar"):
                ents = dump[table + ".Entity"][0].view(np.int32).reshape(-1, 2)
                gens.update({int(i): int(g) for g, i in ents})
            status, count, hits = _out(q.compute())
            assert not status.any()
            hits = hits.reshape(W, G, K, 2)
            count = count.reshape(W, G)
            assert count.max() <= K
            for w, body in enumerate(bodies):
                half = body["scale"] * np.float32(0.5)
                b_lo, b_hi = body["pos"] - half, body["pos"] + half
                # (the first build is in step 1, a rebuild in every fourth step)
                after_rebuild = (step == 1 or step % U.PLAN_REBUILD_PERIOD == 0) and \
                    len(body["id"]) > 32
                if after_rebuild:
                    by_leaf = np.argsort(body["leaf"])
                    p_min, p_max = U.leaf_boxes(body["pos"][by_leaf], body["scale"][by_leaf],
                                                body["vel"][by_leaf])
                    tree = U.restated_build(((p_min + p_max) / np.float32(2)).astype(np.float32))
                    rank = {int(body["id"][by_leaf][leaf]): r
                            for r, leaf in enumerate(tree["traversal"])}
                for g in range(G):
                    if len(body["id"]):
                        # the exclusion rule: a condition on the inputs
                        for a in range(3):
                            others = [x for x in range(3) if x != a]
                            decided = np.all(b_hi[:, others] > q_lo[w, g, others], axis=1) & \
                                np.all(q_hi[w, g, others] > b_lo[:, others], axis=1)
                            for face, side in ((q_lo[w, g, a], b_hi[:, a]),
                                               (q_hi[w, g, a], b_lo[:, a])):
                                near = np.abs(side - face) <= 1e-5 * np.maximum(1, np.abs(side))
                                assert not (near & decided).any(), (layout, step, w, g)
                    inside = np.all(b_hi > q_lo[w, g], axis=1) & np.all(q_hi[w, g] > b_lo, axis=1)
                    want = set(int(i) for i in body["id"][inside])
                    got = hits[w, g, :count[w, g]]
                    ids = [int(i) for i in got[:, 1]]
                    assert len(set(ids)) == len(ids), (layout, step, w, g)
                    assert set(ids) == want, (layout, step, w, g)
                    assert count[w, g] == len(want)
                    assert all(gens[i] == int(gen) for gen, i in got)
                    assert (hits[w, g, count[w, g]:] == -1).all()
                    if after_rebuild:
                        ranks = [rank[i] for i in ids]
                        assert ranks == sorted(ranks), (layout, step, w, g)
                        late += any(r >= 32 for r in ranks)
                        big += count[w, g] > 32
        assert late > 0 and big > 0, (late, big)


# ---- 3. mappings agree bit for bit -------------------------------------------------------
def test_mappings_agree_bit_for_bit(built, monkeypatch):
    """The same boxes as bundles of 4, as B bundles of 1 in a fixed shuffled
    order (adjacent groups hold different worlds), as bundles of 40 (chunks of
    32 + 8) and packed: the same status, count and hits."""
    G = 40
    q_lo, q_hi = _random_boxes(13, W, G)
    # (a few bad boxes and an empty one travel along)
    q_lo[3, 5, 1] = np.nan
    q_hi[7, 33] = q_lo[7, 33] - np.float32(1)
    q_hi[9, 2] = q_lo[9, 2]
    B = W * G
    perm = np.random.default_rng(17).permutation(B)
    world_of = np.repeat(np.arange(W, dtype=np.int32), G)
    with _plan("drift", monkeypatch) as s:
        forty = _absolute(s, G)
        packed = _absolute(s, G, packed=True)
        four = s.box_query(B // 4, 4, K)
        single = s.box_query(B, 1, K)
        _set(four.worlds(), world_of[::4])
        _set(single.worlds(), world_of[perm])
        for query in (forty, packed, four):
            _set(query.lo(), q_lo.reshape(-1, 3))
            _set(query.hi(), q_hi.reshape(-1, 3))
        _set(single.lo(), q_lo.reshape(-1, 3)[perm])
        _set(single.hi(), q_hi.reshape(-1, 3)[perm])
        for step in range(1, 7):
            s.step(1)
            want = _out(packed.compute())
            assert (want[0] == BAD_BOX).sum() == 2 and want[1].max() > 32
            _same(_out(forty.compute()), want, ("bundles of 40", step))
            _same(_out(four.compute()), want, ("bundles of 4", step))
            shuffled = _out(single.compute())
            _same(tuple(x[np.argsort(perm)] for x in shuffled), want, ("bundles of 1", step))


def test_mappings_agree_where_bodies_rotate(built):
    """escape_room_phys, 65 worlds, 30 steps of random actions with auto-reset:
    boxes of half extent 0.5, 2 and 8 around each agent, fed from a step view of
    the agents' positions with bundles_per_world and the view's counts; the
    cooperative mapping against the packed one."""
    WORLDS, A, HITS = 65, 2, 48
    rng = np.random.default_rng(21)
    half = np.tile(np.float32([[0.5] * 3, [2] * 3, [8] * 3]), (WORLDS * A, 1))
    with Simulator(hip_lib_path("escape_room_phys"), WORLDS, seed=9, flags=10) as s, \
            s.world_view("Agent", ["Agent.Position"], max_rows=A) as view:
        view.every_step()
        source = dict(centre=(view.buffer_ptr("Agent.Position"), 12, 0), bundles_per_world=A,
                      count=(view.counts_ptr, 4, 0))
        coop = s.box_query(WORLDS * A, 3, HITS, **source)
        packed = s.box_query(WORLDS * A, 3, HITS, packed=True, **source)
        for query in (coop, packed):
            _set(query.lo(), -half)
            _set(query.hi(), half)
        met = 0
        for step in range(30):
            actions = np.stack([rng.integers(0, 4, (WORLDS, A)), rng.integers(0, 8, (WORLDS, A)),
                                rng.integers(-2, 3, (WORLDS, A)), rng.integers(0, 2, (WORLDS, A))],
                               -1).astype(np.int32)
            s.write_tensor("action", actions)
            s.step(1)
            want = _out(packed.compute())
            _same(_out(coop.compute()), want, ("escape_room_phys", step))
            assert not want[0].any()
            met += int(want[1].sum())
            # every agent is inside its own boxes
            assert (want[1] >= 1).all()
        assert met > 30 * WORLDS * A * 3


# ---- 5. before the first step ------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_compute_before_the_first_step(built, monkeypatch, packed):
    """No broadphase pass has built a tree: every box is OK with count 0 and no
    hits, the trees untouched."""
    with _plan("drift", monkeypatch) as s:
        q = _absolute(s, 2, 5, packed=packed)
        _set(q.lo(), np.full((W * 2, 3), -50, np.float32))
        _set(q.hi(), np.full((W * 2, 3), 50, np.float32))
        _set(q.counts(), np.full(W * 2, 77, np.int32))
        _set(q.hits(), np.zeros((W * 2, 5, 2), np.int32))
        status, count, hits = _out(q.compute())
        assert not status.any() and not count.any() and (hits == -1).all()
        s.step(1)
        status, count, hits = _out(q.compute())
        assert not status.any() and count.max() > 100


# ---- 6. nothing is trusted ---------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_nothing_is_trusted(built, monkeypatch, packed):
    """Worlds -1, W and 2^31 - 1; NaN and inf in centre, lo and hi; sums that
    overflow; an inverted box; counts that skip; sources with a stride.  Each
    gives its status, everything else in the launch is what a clean run leaves,
    and fields behind a failed check are poisoned to show they are not read."""
    torch = _torch()
    G, ROWS = 3, 2
    F = W * ROWS
    B = F * G
    nan, inf, big = np.float32(np.nan), np.float32(np.inf), np.float32(3e38)
    rng = np.random.default_rng(3)
    centre = np.stack([rng.uniform(-4, 4, F), rng.uniform(-4, 4, F),
                       rng.uniform(0, 3, F)], -1).astype(np.float32)
    half = rng.uniform(0.5, 4, (B, 3)).astype(np.float32)
    world = np.repeat(np.arange(W, dtype=np.int32), ROWS)
    with _plan("drift", monkeypatch) as s:
        s.step(2)
        # strided sources: world in word 1 of 3, centre in words 2..4 of 6
        wrec = torch.full((F, 3), 12345, dtype=torch.int32, device="cuda")
        crec = torch.full((F, 6), float("nan"), dtype=torch.float32, device="cuda")
        q = s.box_query(F, G, K, world=(wrec.data_ptr(), 12, 4), centre=(crec.data_ptr(), 24, 8),
                        packed=packed)

        def run(worlds, centres, lo, hi):
            wrec[:, 1] = torch.from_numpy(worlds).cuda()
            crec[:, 2:5] = torch.from_numpy(centres).cuda()
            _set(q.lo(), lo)
            _set(q.hi(), hi)
            return _out(q.compute())

        clean = run(world, centre, -half, half)
        assert not clean[0].any() and clean[1].sum() > B

        worlds2, centres2, lo2, hi2 = world.copy(), centre.copy(), -half, half.copy()
        want_status = np.zeros(B, np.int32)

        def bundle(f, code):
            want_status[f * G:(f + 1) * G] = code

        for f, bad in ((0, -1), (5, W), (9, 2**31 - 1)):
            worlds2[f] = bad
            centres2[f] = nan              # (not read)
            lo2[f * G:(f + 1) * G] = nan
            bundle(f, BAD_WORLD)
        centres2[11, 2] = nan
        centres2[12, 0] = inf
        centres2[13, 1] = -inf
        for f in (11, 12, 13):
            lo2[f * G:(f + 1) * G] = nan   # (not read)
            bundle(f, BAD_BOX)
        per_box = {20 * G: ("lo", 0, nan), 21 * G + 1: ("hi", 2, inf), 22 * G + 2: ("lo", 1, -inf),
                   23 * G: ("hi", 0, big), 24 * G + 1: ("lo", 2, -big)}
        centres2[23] = np.float32([3e38, 0, 1])     # the sum overflows
        centres2[24] = np.float32([0, 0, -3e38])
        bundle(23, BAD_BOX)     # (every sum of the bundle: centre + anything finite but
        bundle(24, BAD_BOX)     #  huge stays finite, so only the listed box is bad)
        want_status[23 * G:24 * G] = OK
        want_status[24 * G:25 * G] = OK
        for b, (which, axis, value) in per_box.items():
            (lo2 if which == "lo" else hi2)[b, axis] = value
            want_status[b] = BAD_BOX
        hi2[30 * G + 1, 1] = lo2[30 * G + 1, 1] - np.float32(0.5)      # inverted
        want_status[30 * G + 1] = BAD_BOX
        status, count, hits = run(worlds2, centres2, lo2, hi2)
        assert np.array_equal(status, want_status)
        bad = status != OK
        assert not count[bad].any() and (hits[bad] == -1).all()
        # bundles 23 and 24 moved (their centres changed); everything else is the clean run's
        same = ~bad
        same[23 * G:25 * G] = False
        assert np.array_equal(count[same], clean[1][same])
        assert np.array_equal(hits[same], clean[2][same])
        q.close()

        # counts that skip, with the rule for the world (F = W x ROWS: no bundle's
        # world is out of range here; the next test has some); a skipped bundle's
        # centre is not read
        counts = torch.from_numpy((np.arange(W) % (ROWS + 1)).astype(np.int32)).cuda()
        slab = torch.from_numpy(centre).cuda()
        skip_rows = (np.arange(F) % ROWS) >= np.repeat(np.arange(W) % (ROWS + 1), ROWS)
        poisoned = centre.copy()
        poisoned[skip_rows] = nan
        slab.copy_(torch.from_numpy(poisoned).cuda())
        torch.cuda.synchronize()
        with s.box_query(F, G, K, centre=slab, bundles_per_world=ROWS, count=counts,
                         packed=packed) as ruled:
            _set(ruled.lo(), -half)
            _set(ruled.hi(), half)
            with pytest.raises(RuntimeError):
                ruled.worlds()
            with pytest.raises(RuntimeError):
                ruled.centres()
            status, count, hits = _out(ruled.compute())
            skipped = np.repeat(skip_rows, G)
            assert skipped.any() and not skipped.all()
            assert np.array_equal(status, np.where(skipped, SKIPPED, OK))
            assert not count[skipped].any() and (hits[skipped] == -1).all()
            assert np.array_equal(count[~skipped], clean[1][~skipped])
            assert np.array_equal(hits[~skipped], clean[2][~skipped])


@pytest.mark.parametrize("packed", [False, True])
def test_a_bad_world_by_the_rule_comes_before_its_count(built, monkeypatch, packed):
    """bundles_per_world with more bundles than W x bundles_per_world: the
    bundles past the last world are BAD_WORLD, and the count source, which has
    exactly W records with poison behind them, is not indexed by their world.
    (A count read there would be 0x7FFFFFFF: not SKIPPED but, worse, a centre
    read and a tree of a world that does not exist.)"""
    torch = _torch()
    ROWS, EXTRA, G = 2, 5, 2
    F = W * ROWS + EXTRA
    counts = torch.full((W + 4,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    counts[:W] = torch.from_numpy((np.arange(W) % (ROWS + 1)).astype(np.int32)).cuda()
    centre = np.zeros((F, 3), np.float32)
    centre[W * ROWS:] = np.nan      # (not read)
    slab = torch.from_numpy(centre).cuda()
    torch.cuda.synchronize()
    with _plan("drift", monkeypatch) as s:
        s.step(2)
        with s.box_query(F, G, 8, centre=slab, bundles_per_world=ROWS, count=counts,
                         packed=packed) as q:
            _set(q.lo(), np.full((F * G, 3), -50, np.float32))
            _set(q.hi(), np.full((F * G, 3), 50, np.float32))
            status, count, hits = _out(q.compute())
            want = np.where((np.arange(W * ROWS) % ROWS) >= np.repeat(np.arange(W) % (ROWS + 1),
                                                                       ROWS), SKIPPED, OK)
            want = np.repeat(np.concatenate([want, np.full(EXTRA, BAD_WORLD)]), G)
            assert np.array_equal(status, want)
            assert not count[want != OK].any() and (hits[want != OK] == -1).all()
            assert count[want == OK].max() > 100


def test_a_handle_of_another_executor_is_refused(built):
    """Every entry point looks the query up in ITS executor first: another
    executor's live handle is -3 there, and the query is left as it was."""
    import ctypes as C
    rt = runtime_lib()
    lib = hip_lib_path("broadphase_only")
    with Simulator(lib, 3, seed=3, flags=1) as s, Simulator(lib, 3, seed=3, flags=1) as other:
        s.step(1)
        other.step(1)
        q = s.box_query(3, 2, 4)
        foreign = other.hip_exec()
        for call in (lambda: rt.mwhip_boxes_compute(foreign, q.handle),
                     lambda: rt.mwhip_boxes_compute_async(foreign, q.handle),
                     lambda: rt.mwhip_set_step_boxes(foreign, q.handle, 1),
                     lambda: rt.mwhip_set_step_boxes(foreign, q.handle, 0)):
            assert call() == -3
            assert "box query %d is not one of this executor's" % q.handle in \
                rt.mwhip_last_error().decode()
        nbytes = C.c_uint64(5)
        assert rt.mwhip_boxes_buffer(foreign, q.handle, 4, C.byref(nbytes)) is None
        assert nbytes.value == 5
        rt.mwhip_boxes_destroy(foreign, q.handle)       # (not its own: nothing happens)
        assert "boxes:boxes" not in [k["name"] for k in other.profile(1)]
        q.compute()
        assert rt.mwhip_boxes_buffer(s.hip_exec(), q.handle, 4, C.byref(nbytes)) is not None
        assert nbytes.value == 3 * 2 * 4
        handle = q.handle
        q.close()
        assert rt.mwhip_boxes_compute(s.hip_exec(), handle) == -3      # destroyed


def test_a_step_box_query_does_not_keep_the_carried_refresh(built):
    """escape_room_phys and a twin, 10 steps to settle; then a step box query
    on one of them.  Behind the one full replay that follows the change of the
    launch graphs, eight more replays leave out the carried leaf refresh as often
    as the twin's do, which has no query; and they do leave it out."""
    WORLDS, A = 65, 2
    lib = hip_lib_path("escape_room_phys")
    with Simulator(lib, WORLDS, seed=5, flags=40) as s, \
            Simulator(lib, WORLDS, seed=5, flags=40) as twin:
        for sim in (s, twin):
            sim.step_async(10)
            sim.sync()
        q = s.box_query(WORLDS * A, 1, 4)
        _set(q.worlds(), np.repeat(np.arange(WORLDS, dtype=np.int32), A))
        _set(q.lo(), np.full((WORLDS * A, 3), -30, np.float32))
        _set(q.hi(), np.full((WORLDS * A, 3), 30, np.float32))
        q.every_step()
        for sim in (s, twin):
            sim.step_async(1)
            sim.sync()
        before = (s.broadphase_stats(), twin.broadphase_stats())
        for sim in (s, twin):
            sim.step_async(8)
            sim.sync()
        after = (s.broadphase_stats(), twin.broadphase_stats())
        carried = [a["carried_replays"] - b["carried_replays"] for a, b in zip(after, before)]
        full = [a["full_replays"] - b["full_replays"] for a, b in zip(after, before)]
        assert carried[0] == carried[1] and full[0] == full[1], (before, after)
        assert carried[0] >= 4 and carried[0] + full[0] == 8, (before, after)
        assert _out(q)[1].max() > 0
        assert "boxes:boxes" in [k["name"] for k in s.profile(1)]


# ---- 7. step stage and lifecycle ---------------------------------------------------------
def test_step_stage_records_a_trail_and_feeds_a_gather(built):
    """every_step() with a step view feeding the centres, a step gather of
    Position over the hits and an output ring over count: 6 queued replays
    leave the trail and the gathered positions of a twin stepped one by one
    with compute() called by hand."""
    torch = _torch()
    rt = runtime_lib()
    WORLDS, STEPS, ROWS, G, HITS = 7, 6, 3, 2, 24
    F = WORLDS * ROWS
    B = F * G
    half = np.tile(np.float32([[1] * 3, [4] * 3]), (F, 1))

    def make(sim):
        view = sim.world_view("Sensor", ["Sensor.Position"], max_rows=ROWS)
        q = sim.box_query(F, G, HITS, centre=(view.buffer_ptr("Sensor.Position"), 12, 0),
                          bundles_per_world=ROWS, count=(view.counts_ptr, 4, 0))
        _set(q.lo(), -half)
        _set(q.hi(), half)
        gather = sim.entity_gather(q.handle_source(), ["Position"])
        return view, q, gather

    lib = hip_lib_path("broadphase_only")
    with Simulator(lib, WORLDS, seed=3, flags=1) as s, Simulator(lib, WORLDS, seed=3,
                                                                 flags=1) as twin:
        base = [k["name"] for k in s.profile(1)]
        twin.step(1)
        assert "boxes:boxes" not in base
        view, q, gather = make(s)
        t_view, t_q, t_gather = make(twin)
        view.every_step()
        q.every_step()
        gather.every_step()
        ring = torch.full((STEPS, B), 99, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert rt.mwhip_set_output_ring(s.hip_exec(), q.buffer_ptr("count"), ring.data_ptr(),
                                        B * 4, STEPS, RING_ON_STEP) == 0
        s.step_async(STEPS)
        trail = np.zeros((STEPS, B), np.int32)
        for k in range(STEPS):
            twin.step(1)
            t_view.compute()
            want = _out(t_q.compute())
            t_gather.compute()
            trail[k] = want[1]
            want_pos = t_gather.tensor("Position", np.float32).cpu().numpy().copy()
        s.sync()
        assert np.array_equal(ring.cpu().numpy(), trail)
        assert trail.max() > 0 and not np.array_equal(trail[0], trail[STEPS - 1])
        _same(_out(q), want, "the last replay")
        assert (want[0] == SKIPPED).any() and (want[0] == OK).any()
        got_pos = gather.tensor("Position", np.float32).cpu().numpy()
        assert np.array_equal(got_pos.view(np.int32), want_pos.view(np.int32))
        # one launch, behind the view and in front of the gather and the ring
        during = [k["name"] for k in s.profile(1)]
        at = during.index("boxes:boxes")
        assert during.count("boxes:boxes") == 1
        assert during[at - 1] == "view:view" and during[at + 1] == "gather:gather", during
        assert during[at + 2] == "ring:ring.out"
        assert rt.mwhip_set_output_ring(s.hip_exec(), q.buffer_ptr("count"), None, 0, 0,
                                        RING_ON_STEP) == 0
        gather.close()
        q.close()
        view.every_step(False)
        assert [k["name"] for k in s.profile(1)] == base


def test_lifecycle(built, monkeypatch):
    with _plan("drift", monkeypatch, worlds=6) as s:
        s.step(3)
        q_lo, q_hi = _random_boxes(5, 6, 4)
        with s.box_query(6, 4, K) as q, s.snapshot() as snap:
            _set(q.worlds(), np.arange(6, dtype=np.int32))
            _set(q.lo(), q_lo.reshape(-1, 3))
            _set(q.hi(), q_hi.reshape(-1, 3))
            at_save = _out(q.compute())
            _same(at_save, _out(q.compute()), "compute() twice")
            snap.save()
            s.step(5)
            later = _out(q.compute())
            snap.restore()
            _same(later, _out(q), "derived state: not restored")
            _same(at_save, _out(q.compute()), "restored and computed")

            # a fifth step query is refused; destroying a set one unsets it
            before = [k["name"] for k in s.profile(1)]
            assert "boxes:boxes" not in before
            more = [s.box_query(2, 3, 4) for _ in range(4)]
            q.every_step()
            for m in more[:3]:
                m.every_step()
            assert [k["name"] for k in s.profile(1)].count("boxes:boxes") == 1
            with pytest.raises(RuntimeError, match=r"-> -2.*at most 4"):
                more[3].every_step()
            more[0].close()
            more[3].every_step()
            s.step(2)
            for m in more[1:]:
                m.close()
            assert [k["name"] for k in s.profile(1)].count("boxes:boxes") == 1
        assert [k["name"] for k in s.profile(1)] == before
        assert s._box_queries == []

        # the creation limits, each refused with -2 before anything is allocated
        for args in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (2**16, 2**8, 2**7), (2**31, 1, 1)):
            with pytest.raises(RuntimeError, match=r"-> -2"):
                s.box_query(*[a & 0xFFFFFFFF for a in args])
        with pytest.raises(RuntimeError, match=r"-> -2.*bundles_per_world"):
            s.box_query(4, 1, 1, count=(s.box_query(1, 1, 1).buffer_ptr("count"), 4, 0))
        with pytest.raises(RuntimeError, match=r"-> -2.*multiples of 4"):
            s.box_query(4, 1, 1, centre=(s.box_query(1, 1, 1).buffer_ptr("lo") + 2, 12, 0))

    # a simulator without a broadphase registered no kernel
    with Simulator(hip_lib_path("cartpole"), 4) as s:
        with pytest.raises(RuntimeError, match=r"-> -2.*registered no box kernel"):
            s.box_query(4, 1, 1)
