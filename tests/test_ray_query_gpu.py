"""Ray queries (mwhip_rays_*, Simulator.ray_query) on the device.
The yardstick is the simulators' own ray systems, which are in lock step with
the reference (test_parity_gpu.py, test_bvh_edges_gpu.py): broadphase_only's
Sensor.RayFan / RayFanPlain and escape_room_phys's exported lidar tensor.  A
query that is given the same worlds, origins, directions and t_max must leave
the same words.  Directions come from the float32 restatement of
madrona_amd/ray_ref.py, pinned by tests/test_ray_directions.py."""
import ctypes as C

import numpy as np
import pytest

from bvh_edges_utils import PLAIN_RAYS, RAY_T_MAX, plan_flags
from madrona_amd import ray_ref
from madrona_amd.simlib import RING_ON_STEP, Simulator, hip_lib_path, runtime_lib
from ray_utils import lidar_table

pytestmark = pytest.mark.gpu

HIT, MISS, SKIPPED, BAD_WORLD, BAD_RAY = 1, 0, -1, -2, -3
R = 32      # consts::raysPerSensor


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bp(worlds, flags=1, seed=3):
    return Simulator(hip_lib_path("broadphase_only"), worlds, seed=seed, flags=flags)


BP_COLUMNS = ("Sensor.Position", "Sensor.RayFan", "Box.LeafID")


def _dump(sim, names=BP_COLUMNS):
    """The named columns alone (a dump of every column makes room for thousands
    of candidate pairs per world)."""
    listed = [c[0] for c in sim.columns]
    return {name: sim.dump_column(listed.index(name), 256) for name in names}


def _sensors(dump, num_worlds):
    """(world int32 [F], origin float32 [F, 3], RayFan int32 [F, 160], RayFanPlain
    int32 [F, 40] or None) of a broadphase_only dump, world by world"""
    pos, counts = dump["Sensor.Position"]
    assert len(counts) == num_worlds
    worlds = np.repeat(np.arange(num_worlds, dtype=np.int32), counts)
    fan = dump["Sensor.RayFan"][0].view(np.int32).reshape(-1, 160)
    plain = dump["Sensor.RayFanPlain"][0].view(np.int32).reshape(-1, 40) \
        if "Sensor.RayFanPlain" in dump else None
    return worlds, pos.view(np.float32).reshape(-1, 3).copy(), fan, plain


def _set(tensor, values):
    """Writes a query's tensor and WAITS: torch's stream against the executor's
    (which is non-blocking) is the caller's to order, and every compute or step
    behind this reads what was written."""
    torch = _torch()
    tensor.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(tensor.device))
    torch.cuda.synchronize()


def _fill(tensor, value):
    """tensor.fill_(value), ordered like _set"""
    tensor.fill_(value)
    _torch().cuda.synchronize()


def _out(q):
    """(hit_t as int32 bits [N], hit int32 [N, 2], normal as int32 bits [N, 3],
    status int32 [N])"""
    _torch().cuda.synchronize()
    return (q.hit_t().cpu().numpy().view(np.int32), q.hits().cpu().numpy(),
            q.normals().cpu().numpy().view(np.int32), q.status().cpu().numpy())


def _same_as_fan(out, fan, what, rays=None):
    """out of F fans of len(rays) rays against RayFan rows [F, 160] (32 t, 32
    entity ids, 96 normal words), or RayFanPlain rows [F, 40] when rays is
    PLAIN_RAYS' positions"""
    F = fan.shape[0]
    per = fan.shape[1] // 5
    rays = np.arange(per) if rays is None else np.asarray(rays)
    hit_t, hit, normal, status = out
    n = len(rays)
    want_t = fan[:, :per][:, rays]
    want_id = fan[:, per:2 * per][:, rays]
    want_n = fan[:, 2 * per:].reshape(F, per, 3)[:, rays]
    for got, want, name in ((hit_t.reshape(F, n), want_t, "hit_t"),
                            (hit.reshape(F, n, 2)[..., 1], want_id, "hit.id"),
                            (normal.reshape(F, n, 3), want_n, "normal"),
                            (status.reshape(F, n), (want_id >= 0).astype(np.int32), "status")):
        bad = np.argwhere(got != want)
        assert bad.size == 0, (what, name, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
    # a hit names a live generation, a miss Entity::none()
    gens = hit.reshape(F, n, 2)[..., 0]
    assert ((gens == -1) == (want_id < 0)).all(), what


# ---- 1 + 2. the simulator's own fans, and the same rays packed ---------------------------
@pytest.mark.parametrize("worlds", [5, 37])
def test_fans_equal_the_simulators_own_rays_however_they_are_packed(built, worlds):
    """Every step of 20 (the rebuild at step 16 inside): a query of F = the
    Sensor rows fans of 32 rays, world and origin from the dump, leaves the
    words of Sensor.RayFan -- through traceRayShared, a group of 32 lanes per
    fan.  The same rays as N independent fans of one ray in a fixed shuffled
    order (adjacent lanes hold different worlds; plain traceRay, a ray per lane)
    and as fans of 4 (packed as well) leave the same words."""
    directions = ray_ref.fan_directions(False)
    with _bp(worlds) as s:
        s.step(1)
        world, origin, fan, _ = _sensors(_dump(s), worlds)
        F = len(world)
        N = F * R
        perm = np.random.default_rng(11).permutation(N)
        with s.ray_query(F, R) as q, s.ray_query(N, 1) as single, s.ray_query(F * 8, 4) as four:
            assert q.t_max().cpu().numpy().tolist() == [np.inf] * N     # at creation
            assert (q.hits().cpu().numpy() == -1).all() and not q.status().cpu().numpy().any()
            _set(q.directions(), np.tile(directions, (F, 1)))
            _set(single.directions(), np.tile(directions, (F, 1))[perm])
            _set(four.directions(), np.tile(directions, (F, 1)))
            for query in (q, single, four):
                _fill(query.t_max(), RAY_T_MAX)
            hits = 0
            leaves = []
            for step in range(1, 21):
                if step > 1:
                    s.step(1)
                dump = _dump(s)
                world, origin, fan, _ = _sensors(dump, worlds)
                leaves.append(dump["Box.LeafID"][1] + 4)
                _set(q.worlds(), world)
                _set(q.origins(), origin)
                out = _out(q.compute())
                _same_as_fan(out, fan, ("fans", step))
                hits += int((out[3] == HIT).sum())

                _set(single.worlds(), np.repeat(world, R)[perm])
                _set(single.origins(), np.repeat(origin, R, axis=0)[perm])
                shuffled = _out(single.compute())
                for a, b, name in zip(out, shuffled, ("hit_t", "hit", "normal", "status")):
                    unshuffled = np.empty_like(b)
                    unshuffled[perm] = b
                    assert np.array_equal(a, unshuffled), ("one ray per fan", step, name)

                _set(four.worlds(), np.repeat(world, 8))
                _set(four.origins(), np.repeat(origin, 8, axis=0))
                for a, b, name in zip(out, _out(four.compute()),
                                      ("hit_t", "hit", "normal", "status")):
                    assert np.array_equal(a, b), ("fans of four", step, name)
            leaves = np.concatenate(leaves)
            assert leaves.max() > 64 and leaves.min() < 32
            assert hits > 20 * worlds * 8, "the rays do meet boxes"
            assert ((out[3] == HIT) | (out[3] == MISS)).all()


# ---- 3. edge trees ------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["drift", "coincident"])
def test_edge_trees(built, monkeypatch, layout):
    """Plan mode, 29 worlds (the 28-entry leaf table: 0, 1, 2, 64, 65, 129 and 130
    leaves among them), 9 steps, a rebuild every 4: against the fan cast through
    traceRayShared (RayFan) and against the 8 rays the simulator casts through
    plain traceRay (RayFanPlain), by a query of 32-ray fans and by one of
    single rays."""
    W = 29
    # (130 coincident boxes make 8385 candidate pairs: the standalone broadphase's
    # table needs the room every plan-mode test gives it)
    monkeypatch.setenv("MADRONA_MWHIP_MAX_CANDIDATES_PER_WORLD", "2048")
    directions = ray_ref.fan_directions(True)
    with _bp(W, flags=plan_flags(layout), seed=5) as s:
        s.step(1)
        world, origin, fan, plain = _sensors(_dump(s, BP_COLUMNS + ("Sensor.RayFanPlain",)), W)
        F = len(world)
        P = len(PLAIN_RAYS)
        with s.ray_query(F, R) as q, s.ray_query(F * P, 1) as single:
            _set(q.directions(), np.tile(directions, (F, 1)))
            _set(single.directions(), np.tile(directions[PLAIN_RAYS], (F, 1)))
            _fill(q.t_max(), RAY_T_MAX)
            _fill(single.t_max(), RAY_T_MAX)
            hits = 0
            for step in range(1, 10):
                if step > 1:
                    s.step(1)
                world, origin, fan, plain = _sensors(_dump(s, BP_COLUMNS + ("Sensor.RayFanPlain",)), W)
                _set(q.worlds(), world)
                _set(q.origins(), origin)
                out = _out(q.compute())
                _same_as_fan(out, fan, (layout, "RayFan", step))
                picked = tuple(o.reshape((F, R) + o.shape[1:])[:, PLAIN_RAYS] for o in out)
                _same_as_fan(picked, plain, (layout, "RayFanPlain, picked", step))
                _set(single.worlds(), np.repeat(world, P))
                _set(single.origins(), np.repeat(origin, P, axis=0))
                _same_as_fan(_out(single.compute()), plain, (layout, "RayFanPlain", step))
                # the world without a leaf: nothing to meet
                empty = np.repeat(world == 0, R)
                assert empty.any() and (out[3][empty] == MISS).all()
                hits += int((out[3] == HIT).sum())
            assert hits > 0


# ---- 4 + 5. view-fed, queued, recorded; hits feed a gather in the same replay ------------
def test_view_fed_queued_and_the_hits_feed_a_gather_in_the_same_replay(built):
    """A step view of Sensor.Position (3 rows per world) is the origin, its
    counts skip the fans of sensors that do not exist; output rings record hit_t
    and status of 6 queued steps; each slot equals the RayFan of a twin stepped
    by hand.  A step gather over the hits runs behind the query in the same
    replay: for every HIT its world is the ray's and its archetype Box or
    Pillar, for everything else it reports no entity.  (The gather lists LeafID,
    which both body tables have, not ResponseType: a gather names a component
    by a dump-list column, and broadphase_only's dump list has no ResponseType
    column.  World and archetype, which the check is about, need no column.)"""
    torch = _torch()
    rt = runtime_lib()
    W, K, ROWS = 7, 6, 3
    F = W * ROWS
    N = F * R
    directions = np.tile(ray_ref.fan_directions(False), (F, 1))
    with _bp(W) as s, _bp(W) as twin, \
            s.world_view("Sensor", ["Sensor.Position"], max_rows=ROWS) as view:
        base = [k["name"] for k in s.profile(1)]
        twin.step(1)
        assert "rays:rays" not in base
        view.every_step()
        q = s.ray_query(F, R, origin=(view.buffer_ptr("Sensor.Position"), 12, 0),
                        fans_per_world=ROWS, count=(view.counts_ptr, 4, 0))
        _set(q.directions(), directions)
        _fill(q.t_max(), RAY_T_MAX)
        with pytest.raises(RuntimeError):
            q.worlds()          # (the rule replaces the buffer)
        with pytest.raises(RuntimeError):
            q.origins()         # (a source was given)
        gather = s.entity_gather(q.handle_source(), ["LeafID"])
        q.every_step()
        gather.every_step()
        ring_t = torch.zeros((K, N), dtype=torch.float32, device="cuda")
        ring_s = torch.full((K, N), 99, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for name, ring in (("hit_t", ring_t), ("status", ring_s)):
            assert rt.mwhip_set_output_ring(s.hip_exec(), q.buffer_ptr(name), ring.data_ptr(),
                                            N * 4, K, RING_ON_STEP) == 0
        s.step_async(K)
        want_t = np.zeros((K, W, ROWS, R), np.int32)
        want_s = np.full((K, W, ROWS, R), SKIPPED, np.int32)
        for k in range(K):
            twin.step(1)
            dump = _dump(twin)
            world, _, fan, _ = _sensors(dump, W)
            counts = dump["Sensor.Position"][1]
            row = np.concatenate([np.arange(c) for c in counts])
            want_t[k, world, row] = fan[:, :R]
            want_s[k, world, row] = fan[:, R:2 * R] >= 0
        s.sync()
        assert (counts < ROWS).any() and (counts == ROWS).any()
        assert (want_s == SKIPPED).any() and (want_s == HIT).any()
        got_t = ring_t.cpu().numpy().view(np.int32).reshape(want_t.shape)
        got_s = ring_s.cpu().numpy().reshape(want_s.shape)
        for k in range(K):
            assert np.array_equal(got_s[k], want_s[k]), ("status, slot", k)
            assert np.array_equal(got_t[k], want_t[k]), ("hit_t, slot", k)
        assert not np.array_equal(got_t[0], got_t[K - 1]), "nothing moved"
        # the buffers hold the last step's; skipped fans are all zero / none
        hit_t, hit, normal, status = _out(q)
        assert np.array_equal(status, want_s[K - 1].ravel())
        skipped = status == SKIPPED
        assert not hit_t[skipped].any() and not normal[skipped].any()
        assert (hit[skipped] == -1).all()

        # the gather of the same replay
        archetypes = gather.archetypes.cpu().numpy()
        gworlds = gather.worlds.cpu().numpy()
        ids = {}
        for table in ("Box", "Pillar"):
            arch, comp = C.c_uint32(0), C.c_uint32(0)
            idx = [c[0] for c in s.columns].index(table + ".Entity")
            assert s.lib.sim_hip_column_ids(s.handle, idx, C.byref(arch), C.byref(comp)) == 0
            ids[table] = arch.value
        is_hit = status == HIT
        ray_world = np.repeat(np.arange(F) // ROWS, R)
        assert np.array_equal(gworlds[is_hit], ray_world[is_hit])
        assert np.isin(archetypes[is_hit], list(ids.values())).all()
        assert is_hit.any()
        assert (archetypes[~is_hit] == -1).all() and (gworlds[~is_hit] == -1).all()
        leaf = gather.tensor("LeafID", np.int32).cpu().numpy().ravel()
        assert (leaf[is_hit] >= 0).all() and (leaf[is_hit] < 104).all()
        assert not leaf[~is_hit].any()

        # one launch, behind the view and in front of the gather and the rings
        during = [k["name"] for k in s.profile(1)]
        at = during.index("rays:rays")
        assert during.count("rays:rays") == 1
        assert during[at - 1] == "view:view" and during[at + 1] == "gather:gather", during
        assert during[at + 2] == "ring:ring.out"
        for name in ("hit_t", "status"):
            assert rt.mwhip_set_output_ring(s.hip_exec(), q.buffer_ptr(name), None, 0, 0,
                                            RING_ON_STEP) == 0
        gather.close()
        q.close()
        view.every_step(False)
        assert [k["name"] for k in s.profile(1)] == base


# ---- 6. the lidar from Python ------------------------------------------------------------
def test_lidar_from_python(built):
    """escape_room_phys, 24 worlds, 12 steps with resets: rays built from the
    agents' Position (+ 0.5 up) and Rotation with R = 30 and t_max 200, a gather
    of EntityType over the hits; hit_t / 200 and type / NumTypes equal the
    exported lidar tensor bit for bit.  (No node behind lidarSystem moves a body
    or touches the tree: it and collectObservationsSystem close the step, behind
    the step's last broadphase.)"""
    W, A, S, NUM_TYPES = 24, 2, 30, 6
    table = lidar_table()
    rng = np.random.default_rng(4)
    with Simulator(hip_lib_path("escape_room_phys"), W, seed=9, flags=10) as s, \
            s.ray_query(W * A, S) as q:
        gather = s.entity_gather(q.handle_source(), ["EntityType"])
        _fill(q.t_max(), 200.0)
        _set(q.worlds(), np.repeat(np.arange(W, dtype=np.int32), A))
        seen_types = set()
        for step in range(12):
            actions = np.stack([rng.integers(0, 4, (W, A)), rng.integers(0, 8, (W, A)),
                                rng.integers(-2, 3, (W, A)), rng.integers(0, 2, (W, A))],
                               -1).astype(np.int32)
            s.write_tensor("action", actions)
            s.step(1)
            dump = s.dump_all()
            pos, counts = dump["Agent.Position"]
            assert (counts == A).all()
            pos = pos.view(np.float32).reshape(W * A, 3)
            rot = dump["Agent.Rotation"][0].view(np.float32).reshape(W * A, 4)
            _set(q.origins(), pos + np.float32([0, 0, 0.5]))
            _set(q.directions(), ray_ref.normalize_f32(
                ray_ref.rotate_vec_f32(rot[:, None, :], table[None, :, :])).reshape(-1, 3))
            hit_t, _, _, status = _out(q.compute())
            gather.compute()
            types = gather.tensor("EntityType", np.uint32).cpu().numpy().ravel()
            is_hit = status == HIT
            assert (is_hit | (status == MISS)).all()
            assert (gather.archetypes.cpu().numpy()[is_hit] >= 0).all()
            depth = hit_t.view(np.float32) / np.float32(200)
            kind = types.astype(np.float32) / np.float32(NUM_TYPES)
            want = s.read_tensor("lidar").reshape(W * A * S, 2).view(np.int32)
            got = np.stack([depth, kind], -1).astype(np.float32).view(np.int32)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (step, bad[:4], got[bad[0][0]], want[bad[0][0]])
            assert not got[~is_hit].any()
            seen_types |= set(types[is_hit].tolist())
        assert len(seen_types) >= 2, seen_types
        gather.close()


# ---- 7. nothing trusted ------------------------------------------------------------------
@pytest.mark.parametrize("rays", [32, 2])
def test_nothing_is_trusted(built, rays):
    """Bad worlds, a NaN origin, an inf / zero direction and a NaN t_max mixed
    among good rays; world and origin sit in a tensor with guard bytes on both
    sides, at a 16-byte stride behind a 4-byte offset.  Statuses as defined, the
    neighbours as if the bad ones were not there, guards intact, no error flag."""
    torch = _torch()
    W = 5
    directions = ray_ref.fan_directions(False)[:rays]
    with _bp(W) as s:
        s.step(3)
        world, origin, fan, _ = _sensors(_dump(s), W)
        good = len(world)
        bad_worlds = [-1, W, -2 ** 31, 2 ** 31 - 1]
        F = good + len(bad_worlds) + 2
        GUARD = 16      # words
        # record f: [poison, x, y, z] for origins, [poison, world, poison, poison]
        origins = np.full((F, 4), np.nan, np.float32)
        origins[:good, 1:] = origin
        origins[good:good + 4, 1:] = origin[0]
        origins[good + 4, 1:] = [np.nan, 0, 0]
        origins[good + 5, 1:] = [0, 0, -np.inf]
        worlds_rec = np.full((F, 4), 0x7FFFFFF0, np.int32)
        worlds_rec[:good, 1] = world
        worlds_rec[good:good + 4, 1] = bad_worlds
        worlds_rec[good + 4:, 1] = 0
        guard = np.full(GUARD, 0x5A5A5A5A, np.int32)
        obuf = torch.from_numpy(np.concatenate([guard, origins.view(np.int32).ravel(),
                                                guard])).cuda()
        wbuf = torch.from_numpy(np.concatenate([guard, worlds_rec.ravel(), guard])).cuda()
        with s.ray_query(F, rays, world=(wbuf.data_ptr() + 4 * GUARD, 16, 4),
                         origin=(obuf.data_ptr() + 4 * GUARD, 16, 4)) as q:
            d = np.tile(directions, (F, 1)).reshape(F, rays, 3)
            t_max = np.full((F, rays), RAY_T_MAX, np.float32)
            d[1, 0] = [np.inf, 0, 0]
            d[1, rays - 1] = [0, 0, 0]
            d[2, 1] = [0, np.nan, 1]
            t_max[0, 1] = np.nan
            t_max[2, 0] = np.inf        # (not bad: a reach like any other)
            bad_ray = np.zeros((F, rays), bool)
            bad_ray[1, 0] = bad_ray[1, rays - 1] = bad_ray[2, 1] = bad_ray[0, 1] = True
            _set(q.directions(), d.reshape(-1, 3))
            _set(q.t_max(), t_max.ravel())
            first = _out(q.compute())
            hit_t, hit, normal, status = (o.reshape((F, rays) + o.shape[1:]) for o in first)
            assert (status[good:good + 4] == BAD_WORLD).all()
            assert (status[good + 4:] == BAD_RAY).all()
            assert (status[:good][bad_ray[:good]] == BAD_RAY).all()
            for o in (hit_t, normal):
                assert not o[status < 0].any()
            assert (hit[status < 0] == -1).all()
            # the good rays: RayFan's words (t_max 40 there: the ray that reaches
            # further may only differ by a hit beyond 40)
            ok = ~bad_ray[:good]
            ok[2, 0] = False
            want_t = fan[:, :R][:, :rays]
            want_id = fan[:, R:2 * R][:, :rays]
            want_n = fan[:, 2 * R:].reshape(good, R, 3)[:, :rays]
            assert np.array_equal(hit_t[:good][ok], want_t[ok])
            assert np.array_equal(hit[:good][..., 1][ok], want_id[ok])
            assert np.array_equal(normal[:good][ok], want_n[ok])
            assert np.array_equal(status[:good][ok], (want_id[ok] >= 0).astype(np.int32))
            assert (status[:good][ok] == HIT).any()
            if want_id[2, 0] >= 0:
                assert hit_t[2, 0] == want_t[2, 0] and hit[2, 0, 1] == want_id[2, 0]
            # sources untouched, guards included; twice the same; no error flag
            assert np.array_equal(wbuf.cpu().numpy(), np.concatenate([guard, worlds_rec.ravel(),
                                                                      guard]))
            assert np.array_equal(obuf.cpu().numpy(),
                                  np.concatenate([guard, origins.view(np.int32).ravel(), guard]))
            for a, b in zip(first, _out(q.compute())):
                assert np.array_equal(a, b)
            s.sync()
            s.step(1)


# ---- 8. lifecycle ------------------------------------------------------------------------
def test_lifecycle(built):
    torch = _torch()
    W = 6
    directions = ray_ref.fan_directions(False)
    with _bp(W) as s:
        s.step(3)
        world, origin, fan, _ = _sensors(_dump(s), W)
        F = len(world)
        with s.ray_query(F, R) as q, s.snapshot() as snap:
            _set(q.worlds(), world)
            _set(q.origins(), origin)
            _set(q.directions(), np.tile(directions, (F, 1)))
            _fill(q.t_max(), RAY_T_MAX)
            at_save = _out(q.compute())
            _same_as_fan(at_save, fan, "at the save")
            for a, b in zip(at_save, _out(q.compute())):
                assert np.array_equal(a, b), "compute() twice"
            snap.save()
            s.step(5)
            later = _out(q.compute())
            assert not np.array_equal(later[0], at_save[0]), "no box moved"
            snap.restore()
            # (derived state: the buffers still hold the later one)
            for a, b in zip(later, _out(q)):
                assert np.array_equal(a, b)
            for a, b in zip(at_save, _out(q.compute())):
                assert np.array_equal(a, b), "restored and computed"

            # a fifth step query is refused; destroying a set one unsets it
            before = [k["name"] for k in s.profile(1)]
            assert "rays:rays" not in before
            more = [s.ray_query(2, 3) for _ in range(4)]
            q.every_step()
            for m in more[:3]:
                m.every_step()
            during = [k["name"] for k in s.profile(1)]
            assert during.count("rays:rays") == 1
            with pytest.raises(RuntimeError, match=r"-> -2.*at most 4"):
                more[3].every_step()
            more[0].close()
            more[3].every_step()
            s.step(2)
            for m in more[1:]:
                m.close()
            assert [k["name"] for k in s.profile(1)].count("rays:rays") == 1
        # (closed by the with: a set query)
        assert [k["name"] for k in s.profile(1)] == before
        assert s._ray_queries == []

    # a rebuild of the launch graphs keeps the step stage
    with Simulator(hip_lib_path("escape_room_phys"), 4, seed=2) as s, s.ray_query(4, 5) as q:
        _set(q.worlds(), np.arange(4, dtype=np.int32))
        _set(q.origins(), np.float32([[0, 0, 5]] * 4))
        _set(q.directions(), np.float32([[0, 0, -1], [1, 0, 0], [0, 1, 0], [-1, 0, 0],
                                         [0, -1, 0]] * 4))
        q.every_step()
        ring = torch.zeros((2, 4, 2, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s.set_input_ring("action", ring.data_ptr(), 2)
        assert [k["name"] for k in s.profile(1)].count("rays:rays") == 1
        _fill(q.hit_t(), 0.0)
        s.step(1)
        hit_t, _, normal, status = _out(q)
        # straight down from 5 above the floor: the floor plane, or something on it
        down = status.reshape(4, 5)[:, 0]
        assert (down == HIT).all()
        assert (hit_t.view(np.float32).reshape(4, 5)[:, 0] <= 5).all()
        assert (hit_t.view(np.float32).reshape(4, 5)[:, 0] > 0).all()
        s.set_input_ring("action", 0, 0)

    # no broadphase, no ray kernel, no ray queries
    with Simulator(hip_lib_path("cartpole"), 4) as s:
        with pytest.raises(RuntimeError, match=r"-> -2.*no ray kernel"):
            s.ray_query(1, 1)
        assert s._ray_queries == []


# ---- 9. refusals -------------------------------------------------------------------------
def test_refusals(built):
    from madrona_amd.simlib import RaysDesc, RaySource
    torch = _torch()
    rt = runtime_lib()
    with _bp(3) as s, _bp(3) as other:
        s.step(1)
        exec_ = s.hip_exec()
        buf = torch.zeros(64, dtype=torch.int32, device="cuda")
        ptr = buf.data_ptr()

        def create(fans, rays, fans_per_world=0, world=(None, 0, 0), count=(None, 0, 0),
                   origin=(None, 0, 0)):
            desc = RaysDesc(fans, rays, fans_per_world, 0, RaySource(*world), RaySource(*count),
                            RaySource(*origin))
            out = C.c_uint64(99)
            rc = rt.mwhip_rays_create(exec_, C.byref(desc), C.byref(out))
            return rc, out.value, rt.mwhip_last_error().decode()

        for kwargs, word in (
                (dict(fans=0, rays=4), "0 fans of 4 rays"),
                (dict(fans=4, rays=0), "4 fans of 0 rays"),
                (dict(fans=2 ** 16, rays=2 ** 15), "more than 2147483647 rays"),
                (dict(fans=4, rays=2, world=(ptr + 2, 4, 0)), "world: src"),
                (dict(fans=4, rays=2, world=(ptr, 6, 0)), "multiples of 4"),
                (dict(fans=4, rays=2, world=(ptr, 8, 2)), "multiples of 4"),
                (dict(fans=4, rays=2, world=(ptr, 8, 8)), "do not fit"),
                (dict(fans=4, rays=2, origin=(ptr, 8, 0)), "origin: 12 bytes from byte 0"),
                (dict(fans=4, rays=2, origin=(ptr, 16, 8)), "do not fit"),
                (dict(fans=4, rays=2, count=(ptr, 4, 0)), "needs fans_per_world"),
                (dict(fans=4, rays=2, fans_per_world=2, count=(ptr, 4, 4)), "do not fit")):
            rc, out, message = create(**kwargs)
            assert rc == -2 and out == 99 and word in message, (kwargs, rc, out, message)
        assert rt.mwhip_rays_create(exec_, None, C.byref(C.c_uint64(0))) == -2
        # (the largest query allowed, 2^31 - 1 rays of 44 bytes, fits an MI355X:
        # running out of memory is the path every kind shares, CREATE_FAILED)

        # which buffers are owned; handles: unknown, another executor's, destroyed
        rc, handle, message = create(4, 2, fans_per_world=2, origin=(ptr, 12, 0))
        assert rc == 0 and handle not in (0, 99), message
        nbytes = C.c_uint64(5)
        for which, owned, size in ((0, False, 0), (1, False, 0), (2, True, 96), (3, True, 32),
                                   (4, True, 32), (5, True, 64), (6, True, 96), (7, True, 32)):
            got = rt.mwhip_rays_buffer(exec_, handle, which, C.byref(nbytes))
            assert (got is not None) == owned, which
            if owned:
                assert nbytes.value == size and got % 256 == 0, which
            else:
                assert "is not owned" in rt.mwhip_last_error().decode()
        assert rt.mwhip_rays_buffer(exec_, handle, 8, None) is None
        assert "buffer 8 of 8" in rt.mwhip_last_error().decode()
        assert rt.mwhip_rays_compute(exec_, handle) == 0
        assert rt.mwhip_rays_compute(other.hip_exec(), handle) == -3
        assert "ray query %d is not one of this executor's" % handle in \
            rt.mwhip_last_error().decode()
        rt.mwhip_rays_destroy(other.hip_exec(), handle)     # (not its own: nothing happens)
        assert rt.mwhip_rays_compute_async(exec_, handle) == 0
        rt.mwhip_rays_destroy(exec_, handle)
        for call in (lambda: rt.mwhip_rays_compute(exec_, handle),
                     lambda: rt.mwhip_rays_compute_async(exec_, handle),
                     lambda: rt.mwhip_set_step_rays(exec_, handle, 1)):
            assert call() == -3
            assert "ray query %d is not one of this executor's" % handle in \
                rt.mwhip_last_error().decode()
        assert rt.mwhip_rays_buffer(exec_, handle, 7, None) is None

        # the Python wrapper's own checks
        for source in (buf.cpu(), buf.to(torch.int64), buf.reshape(8, 8)[:, :3]):
            with pytest.raises(TypeError):
                s.ray_query(4, 2, origin=source)
        with pytest.raises(TypeError):
            s.ray_query(4, 2, origin=buf.reshape(32, 2))     # rows of 8 bytes
        s.ray_query(4, 2, origin=buf.reshape(16, 4), world=buf[:4]).compute().close()
        s.sync()
        s.step(1)
        assert s._ray_queries == []


# ---- 10. before the first step ------------------------------------------------------------
@pytest.mark.parametrize("rays", [32, 3])
def test_compute_before_the_first_step(built, rays):
    """No broadphase pass has built a tree yet (a rebuild is pending over node
    memory nobody wrote): create, set rays, compute gives MISS everywhere with
    the trees untouched -- on demand, as a step query in front of the first step's
    own results, and after restoring a snapshot taken before the first step."""
    W = 6
    directions = np.tile(ray_ref.fan_directions(False)[:rays], (W, 1))
    origins = np.float32([[0, 0, 1]] * W)

    def all_miss(out, what):
        hit_t, hit, normal, status = out
        assert (status == MISS).all(), what
        assert not hit_t.any() and not normal.any() and (hit == -1).all(), what

    with _bp(W) as s, s.ray_query(W, rays) as q, s.snapshot() as snap:
        _set(q.worlds(), np.arange(W, dtype=np.int32))
        _set(q.origins(), origins)      # (inside the arena, boxes all around)
        _set(q.directions(), directions)
        _fill(q.t_max(), RAY_T_MAX)
        _fill(q.status(), 77)
        all_miss(_out(q.compute()), "before the first step")
        q.compute_async()
        s.sync()
        all_miss(_out(q), "before the first step, queued")
        snap.save()
        # the step stage runs behind the first step's broadphase: built trees
        q.every_step()
        s.step(1)
        first = _out(q)
        assert (first[3] == HIT).any() and ((first[3] == HIT) | (first[3] == MISS)).all()
        for a, b in zip(first, _out(q.compute())):
            assert np.array_equal(a, b)
        q.every_step(False)
        snap.restore()
        all_miss(_out(q.compute()), "restored to before the first step")
        s.step(1)
        for a, b in zip(first, _out(q.compute())):
            assert np.array_equal(a, b), "the first step once more"
