"""numpy fp32 restatement of the reference's Navmesh (include/madrona/navmesh.inl,
src/common/navmesh.cpp), operation for operation, and of the navmesh_agents
simulator (sims/navmesh_agents) built on it.

* build(): fan triangulation, twice-area weights, Vose alias table (under / over
  stacks popped from the top), edge adjacency (an edge met again links the two
  triangles; a third triangle links to the first one and takes over its side).
* The queries run lane-parallel, one lane per query, like the device kernels:
  every numpy operation below is one fp32 operation of the reference, in its
  order, so the results are bit-identical under -ffp-contract=off.
* Random numbers come from the plain-C Threefry restatement
  (oracle/restate, liboracle_restate.so): oracle_split_i, oracle_sample_i32,
  oracle_bits_to_float01.

Pinned to the reference itself through tests/golden/navmesh_ref.npz
(tests/test_navmesh_cpu.py).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from madrona_amd.simlib import REF_BUILD_DIR

F = np.float32
SENTINEL = np.uint32(0xFFFFFFFF)
FLT_MAX = np.finfo(np.float32).max
THIRD = F(1.0) / F(3.0)
HASH_BASIS = np.uint32(2166136261)
HASH_PRIME = np.uint32(16777619)

# navmesh_agents (sims/navmesh_agents/sim.hpp, meshes.hpp)
AGENTS_PER_WORLD = 4
RESAMPLE_EVERY = 5
BFS_RADIUS2 = F(6.25)
MAX_VERTS, MAX_POLY_IDXS, MAX_POLYS = 128, 256, 64


# ---- Threefry through the C restatement ----------------------------------------
class Rand:
    def __init__(self):
        lib = C.CDLL(os.path.join(REF_BUILD_DIR, "liboracle_restate.so"))
        lib.oracle_split_i.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32)] * 2
        lib.oracle_sample_i32.restype = C.c_int32
        lib.oracle_sample_i32.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_int32]
        lib.oracle_bits_to_float01.restype = C.c_float
        lib.oracle_bits_to_float01.argtypes = [C.c_uint32]
        self.lib = lib
        self._a = C.c_uint32()
        self._b = C.c_uint32()

    def split(self, key, idx):
        self.lib.oracle_split_i(int(key[0]), int(key[1]), int(idx), 0,
                                C.byref(self._a), C.byref(self._b))
        return (self._a.value, self._b.value)

    def init_key(self, seed):
        return self.split((seed, 0), 0)

    def sample_i32(self, key, lo, hi):
        return self.lib.oracle_sample_i32(int(key[0]), int(key[1]), lo, hi)

    def float01(self, bits):
        return F(self.lib.oracle_bits_to_float01(int(bits)))


# ---- builder (reference navmesh.cpp:132-338) -----------------------------------
class Mesh:
    """One built navmesh: vertices (V, 3) f32, tri_idx / adjacency (T, 3) u32,
    tau (T,) f32, alias (T,) u32."""

    def __init__(self, verts, tri_idx, adjacency, tau, alias):
        self.verts = verts
        self.tri_idx = tri_idx
        self.adjacency = adjacency
        self.tau = tau
        self.alias = alias

    @property
    def num_tris(self):
        return len(self.tri_idx)


def build(verts, idxs, offsets, sizes) -> Mesh:
    """initFromPolygons.  The reference finds an edge's first triangle through
    an open-addressing hash table; which slot an edge lands in does not change
    the adjacency, so a dict stands in for it."""
    verts = np.asarray(verts, F).reshape(-1, 3)
    idxs = np.asarray(idxs, np.uint32)
    tris = []
    for off, size in zip(offsets, sizes):
        for k in range(1, int(size) - 1):
            tris.append((idxs[off], idxs[off + k], idxs[off + k + 1]))
    T = len(tris)
    tri_idx = np.array(tris, np.uint32).reshape(T, 3)

    A = verts[tri_idx[:, 0]]
    B = verts[tri_idx[:, 1]]
    Cv = verts[tri_idx[:, 2]]
    ab = B - A
    ac = Cv - A
    cx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    cy = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    cz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    w = np.sqrt(cx * cx + cy * cy + cz * cz)
    # sequential fp32 sum, in triangle order
    wsum = np.add.accumulate(w, dtype=F)[-1] if T else F(0)

    weights = (w * F(T)) / wsum
    weights = [F(x) for x in weights]
    under = [t for t in range(T) if weights[t] < F(1)]
    over = [t for t in range(T) if not weights[t] < F(1)]
    tau = np.zeros(T, F)
    alias = np.zeros(T, np.uint32)
    while under and over:
        u = under.pop()
        o = over.pop()
        tau[u] = weights[u]
        alias[u] = o
        nw = F(F(weights[o] + weights[u]) - F(1))
        weights[o] = nw
        (under if nw < F(1) else over).append(o)
    for idx in under + over:
        tau[idx] = F(1)
        alias[idx] = idx

    adjacency = np.full((T, 3), SENTINEL, np.uint32)
    first = {}
    for t in range(T):
        for e in range(3):
            a = int(tri_idx[t, e])
            b = int(tri_idx[t, (e + 1) % 3])
            key = (min(a, b), max(a, b))
            if key not in first:
                first[key] = (t, e)
            else:
                ot, oe = first[key]
                adjacency[t, e] = ot
                adjacency[ot, oe] = t
    return Mesh(verts.copy(), tri_idx, adjacency, tau, alias)


# ---- lane-parallel queries ---------------------------------------------------------
class Pack:
    """Meshes padded into dense arrays so that lanes can gather from theirs."""

    def __init__(self, meshes):
        self.meshes = meshes
        M = len(meshes)
        self.tmax = max(m.num_tris for m in meshes)
        vmax = max(len(m.verts) for m in meshes)
        self.num_tris = np.array([m.num_tris for m in meshes], np.int64)
        self.verts = np.zeros((M, vmax, 3), F)
        self.tri_idx = np.zeros((M, self.tmax, 3), np.int64)
        self.adjacency = np.full((M, self.tmax, 3), SENTINEL, np.uint32)
        self.tau = np.ones((M, self.tmax), F)
        self.alias = np.zeros((M, self.tmax), np.int64)
        for i, m in enumerate(meshes):
            self.verts[i, :len(m.verts)] = m.verts
            self.tri_idx[i, :m.num_tris] = m.tri_idx
            self.adjacency[i, :m.num_tris] = m.adjacency
            self.tau[i, :m.num_tris] = m.tau
            self.alias[i, :m.num_tris] = m.alias

    def tri_verts(self, mesh, tri):
        """a, b, c (N, 3) of triangle tri[n] of mesh mesh[n]"""
        idx = self.tri_idx[mesh, tri]
        return (self.verts[mesh, idx[:, 0]], self.verts[mesh, idx[:, 1]],
                self.verts[mesh, idx[:, 2]])


def sample(rng: Rand, pack: Pack, mesh, keys):
    """samplePointAndPoly (reference navmesh.inl:5-37) for keys[n] on mesh[n]:
    points (N, 3) f32, polys (N,) u32."""
    mesh = np.asarray(mesh, np.int64)
    N = len(mesh)
    row = np.zeros(N, np.int64)
    p = np.zeros(N, F)
    u = np.zeros(N, F)
    v = np.zeros(N, F)
    for n in range(N):
        key = (int(keys[n][0]), int(keys[n][1]))
        row[n] = rng.sample_i32(rng.split(key, 0), 0, int(pack.num_tris[mesh[n]]))
        pk = rng.split(key, 1)
        p[n] = rng.float01(pk[0] ^ pk[1])
        bk = rng.split(key, 2)
        u[n] = rng.float01(bk[0])
        v[n] = rng.float01(bk[1])
    tri = np.where(p < pack.tau[mesh, row], row, pack.alias[mesh, row])
    flip = (u + v) > F(1)
    u = np.where(flip, F(1) - u, u)
    v = np.where(flip, F(1) - v, v)
    w = (F(1) - u) - v
    a, b, c = pack.tri_verts(mesh, tri)
    pts = (a * u[:, None] + b * v[:, None]) + c * w[:, None]
    return pts.astype(F), tri.astype(np.uint32)


def bfs(pack: Pack, mesh, start, centers, radius2):
    """bfsFromPoly (reference navmesh.inl:55-89), accepting a polygon whose
    centroid lies within sqrt(radius2) of centers[n]: visit orders (N, Tmax)
    and counts (N,)."""
    mesh = np.asarray(mesh, np.int64)
    N = len(mesh)
    lanes = np.arange(N)
    T = pack.num_tris[mesh]
    tmax = pack.tmax
    queue = np.zeros((N, tmax), np.int64)
    visited = np.zeros((N, tmax + 1), bool)
    order = np.zeros((N, tmax), np.uint32)
    count = np.zeros(N, np.int64)
    head = np.zeros(N, np.int64)
    tail = np.zeros(N, np.int64)
    centers = np.asarray(centers, F)

    def inc(i):
        return np.where(i == T - 1, 0, i + 1)

    start = np.asarray(start, np.int64)
    queue[lanes, tail] = start
    tail = inc(tail)
    visited[lanes, start] = True
    while True:
        act = head != tail
        if not act.any():
            break
        poly = queue[lanes, head]
        head = np.where(act, inc(head), head)
        order[lanes[act], count[act]] = poly[act]
        count = count + act

        a, b, c = pack.tri_verts(mesh, poly)
        centroid = ((a + b) + c) * THIRD
        d = centroid - centers
        accept = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= radius2
        go = act & accept
        for i in range(3):
            adj = pack.adjacency[mesh, poly, i]
            adj_i = np.where(adj == SENTINEL, tmax, adj).astype(np.int64)
            add = go & (adj != SENTINEL) & ~visited[lanes, adj_i]
            queue[lanes[add], tail[add]] = adj_i[add]
            tail = np.where(add, inc(tail), tail)
            visited[lanes[add], adj_i[add]] = True
    return order, count


class _Heap:
    """PathFindQueue (reference navmesh.cpp:9-112), one per lane."""

    def __init__(self, N, tmax):
        self.lanes = np.arange(N)
        self.costs = np.full((N, tmax), FLT_MAX, F)
        self.heap = np.zeros((N, tmax), np.int64)
        self.index = np.full((N, tmax), int(SENTINEL), np.int64)
        self.size = np.zeros(N, np.int64)

    def _move_up(self, mask, idx, poly, cost):
        L = self.lanes
        idx = idx.copy()
        go = mask & (idx != 0)
        while go.any():
            parent = np.where(go, (idx - 1) // 2, 0)
            pp = self.heap[L, parent]
            go = go & ~(self.costs[L, pp] <= cost)
            self.heap[L[go], idx[go]] = pp[go]
            self.index[L[go], pp[go]] = idx[go]
            idx = np.where(go, parent, idx)
            go = go & (idx != 0)
        self.heap[L[mask], idx[mask]] = poly[mask]
        self.index[L[mask], poly[mask]] = idx[mask]

    def add(self, mask, poly, cost):
        L = self.lanes
        self.costs[L[mask], poly[mask]] = cost[mask]
        new_idx = self.size.copy()
        self.size = self.size + mask
        self._move_up(mask, new_idx, poly, cost)

    def decrease(self, mask, poly, cost):
        L = self.lanes
        self.costs[L[mask], poly[mask]] = cost[mask]
        idx = np.where(mask, self.index[L, poly], 0)
        self._move_up(mask, idx, poly, cost)

    def remove_min(self, mask):
        L = self.lanes
        root = self.heap[:, 0].copy()
        self.size = self.size - mask
        moved = self.heap[L, np.maximum(self.size, 0)]
        moved_cost = self.costs[L, moved]
        idx = np.zeros(len(L), np.int64)
        go = mask.copy()
        while True:
            child = 2 * idx + 1
            go = go & (child < self.size)
            if not go.any():
                break
            cs = np.where(go, child, 0)
            cp = self.heap[L, cs]
            cc = self.costs[L, cp]
            # the cheaper child, the left one on a tie
            right = cs + 1
            has_r = go & (right < self.size)
            rp = self.heap[L, np.where(has_r, right, 0)]
            rc = self.costs[L, rp]
            pick = has_r & (rc < cc)
            cs = np.where(pick, right, cs)
            cp = np.where(pick, rp, cp)
            cc = np.where(pick, rc, cc)
            go = go & ~(moved_cost < cc)
            self.heap[L[go], idx[go]] = cp[go]
            self.index[L[go], cp[go]] = idx[go]
            idx = np.where(go, cs, idx)
        self.heap[L[mask], idx[mask]] = moved[mask]
        self.index[L[mask], moved[mask]] = idx[mask]
        self.index[L[mask], root[mask]] = int(SENTINEL)
        return root


def dijkstra(pack: Pack, mesh, start, start_pos):
    """dijkstrasFromPoly (reference navmesh.inl:92-163): distances (N, Tmax),
    entry points (N, Tmax, 3; zero where never written), pop orders and the
    distances they were popped with (N, Tmax), pop counts (N,)."""
    mesh = np.asarray(mesh, np.int64)
    N = len(mesh)
    L = np.arange(N)
    tmax = pack.tmax
    start = np.asarray(start, np.int64)
    h = _Heap(N, tmax)
    entry = np.zeros((N, tmax, 3), F)
    order = np.zeros((N, tmax), np.uint32)
    pop_dist = np.zeros((N, tmax), F)
    count = np.zeros(N, np.int64)

    entry[L, start] = np.asarray(start_pos, F)
    everyone = np.ones(N, bool)
    h.add(everyone, start, np.zeros(N, F))
    while True:
        act = h.size > 0
        if not act.any():
            break
        mp = np.where(act, h.remove_min(act), 0)
        cur = entry[L, mp]
        d_so_far = h.costs[L, mp]
        order[L[act], count[act]] = mp[act]
        pop_dist[L[act], count[act]] = d_so_far[act]
        count = count + act

        a, b, c = pack.tri_verts(mesh, mp)
        ends = ((a, b), (b, c), (c, a))
        for i in range(3):
            adj = pack.adjacency[mesh, mp, i]
            valid = act & (adj != SENTINEL)
            adj_i = np.where(valid, adj, 0).astype(np.int64)
            e0, e1 = ends[i]
            mid = (e0 + e1) / F(2)
            dv = cur - mid
            dte = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
            new = d_so_far + dte
            prev = h.costs[L, adj_i]
            upd = valid & ~(new >= prev)
            entry[L[upd], adj_i[upd]] = mid[upd]
            fresh = upd & (h.index[L, adj_i] == int(SENTINEL))
            h.add(fresh, adj_i, new)
            h.decrease(upd & ~fresh, adj_i, new)
    return h.costs, entry, order, pop_dist, count


# ---- navmesh_agents ------------------------------------------------------------------
def agents_polygons(sim_lib, global_world, seed, flags):
    """The polygons of one world, from the simulator library itself
    (sim_navmesh_polygons, sims/navmesh_agents/mgr.cpp)."""
    verts = np.zeros(MAX_VERTS * 3, F)
    idxs = np.zeros(MAX_POLY_IDXS, np.uint32)
    offs = np.zeros(MAX_POLYS, np.uint32)
    sizes = np.zeros(MAX_POLYS, np.uint32)
    counts = np.zeros(3, np.uint32)
    fn = sim_lib.sim_navmesh_polygons
    fn.restype = C.c_int32
    fn.argtypes = [C.c_uint32] * 3 + [C.c_void_p] * 5
    family = fn(global_world, seed, flags, verts.ctypes.data, idxs.ctypes.data,
                offs.ctypes.data, sizes.ctypes.data, counts.ctypes.data)
    nv, ni, npoly = (int(x) for x in counts)
    return (family, verts[:3 * nv].reshape(nv, 3).copy(), idxs[:ni].copy(),
            offs[:npoly].copy(), sizes[:npoly].copy())


def _fnv(h, poly):
    return ((h ^ poly.astype(np.uint32)) * HASH_PRIME).astype(np.uint32)


class AgentsRestatement:
    """navmesh_agents (sims/navmesh_agents/sim.cpp) for the given global world
    indices, one lane per agent (worlds are independent of each other)."""

    def __init__(self, rng: Rand, sim_lib, worlds, seed, flags):
        self.rng = rng
        worlds = [int(w) for w in worlds]
        num_worlds = len(worlds)
        meshes = []
        self.families = []
        self.polygons = []
        for w in worlds:
            fam, v, i, o, s = agents_polygons(sim_lib, w, seed, flags)
            self.families.append(fam)
            self.polygons.append((v, i, o, s))
            meshes.append(build(v, i, o, s))
        self.pack = Pack(meshes)
        A = AGENTS_PER_WORLD
        self.N = num_worlds * A
        self.mesh = np.repeat(np.arange(num_worlds), A)
        self.agent = np.tile(np.arange(A), num_worlds)
        self.world_keys = [rng.split(rng.init_key(seed), w) for w in worlds]
        self.epoch = np.zeros(self.N, np.uint32)
        self.step_idx = np.zeros(self.N, np.uint32)
        self.pos = np.zeros((self.N, 3), F)
        self.poly = np.zeros(self.N, np.uint32)
        self.goal = np.zeros((self.N, 3), F)
        self.goal_poly = np.zeros(self.N, np.uint32)
        self.dij = np.zeros((self.N, 3), np.uint32)    # goalDist bits, popped, hash
        self.bfs_stats = np.zeros((self.N, 2), np.uint32)
        self._resample(np.ones(self.N, bool))

    def _resample(self, mask):
        rng = self.rng
        lanes = np.nonzero(mask)[0]
        pos_keys, goal_keys = [], []
        for n in lanes:
            wk = self.world_keys[self.mesh[n]]
            k = rng.split(rng.split(wk, int(self.epoch[n])), int(self.agent[n]))
            pos_keys.append(rng.split(k, 0))
            goal_keys.append(rng.split(k, 1))
        p, pp = sample(rng, self.pack, self.mesh[lanes], pos_keys)
        g, gp = sample(rng, self.pack, self.mesh[lanes], goal_keys)
        self.pos[lanes] = p
        self.poly[lanes] = pp
        self.goal[lanes] = g
        self.goal_poly[lanes] = gp

    def step(self):
        self.step_idx = self.step_idx + np.uint32(1)
        mask = (self.step_idx % RESAMPLE_EVERY) == 0
        if mask.any():
            self.epoch = self.epoch + mask.astype(np.uint32)
            self._resample(mask)

        dist, _, order, _, count = dijkstra(self.pack, self.mesh, self.poly, self.pos)
        h = np.full(self.N, HASH_BASIS, np.uint32)
        for k in range(self.pack.tmax):
            live = count > k
            h = np.where(live, _fnv(h, order[:, k]), h)
        goal_dist = dist[np.arange(self.N), self.goal_poly.astype(np.int64)]
        self.dij = np.stack([goal_dist.view(np.uint32), count.astype(np.uint32), h], -1)

        border, bcount = bfs(self.pack, self.mesh, self.poly, self.pos, BFS_RADIUS2)
        h = np.full(self.N, HASH_BASIS, np.uint32)
        for k in range(self.pack.tmax):
            live = bcount > k
            h = np.where(live, _fnv(h, border[:, k]), h)
        self.bfs_stats = np.stack([bcount.astype(np.uint32), h], -1)

    def columns(self):
        """rows of the simulator's dump columns, as uint32 words"""
        pos = np.concatenate([self.pos.view(np.uint32), self.poly[:, None]], -1)
        goal = np.concatenate([self.goal.view(np.uint32), self.goal_poly[:, None]], -1)
        info = np.stack([self.agent.astype(np.uint32), self.epoch, self.step_idx], -1)
        return {
            "Agent.NavPosition": pos,
            "Agent.NavGoal": goal,
            "Agent.DijkstraStats": self.dij,
            "Agent.BfsStats": self.bfs_stats,
            "Agent.AgentInfo": info,
        }


def device_block_bytes(num_verts, num_tris):
    """navmesh_detail::deviceBlockBytes (include/madrona/navmesh.inl): the
    persistent-region bytes of one device initFromPolygons"""
    def a128(v):
        return (v + 127) & ~127
    total = a128(12 * num_verts) + a128(12 * num_tris) + a128(12 * num_tris) + 8 * num_tris
    return (total + 112 + 15) & ~15
