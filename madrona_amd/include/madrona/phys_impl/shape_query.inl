// Shape queries (mwhip_shapes_*, include/mwhip.h): posed
// collision shapes that are no table rows, each tested against the rigid bodies
// of its world with the narrowphase of the step; per shape the bodies it would
// touch with the manifold of each, in the order (body k, primitive pair).
// Included by physics.inl inside madrona::phys::kernels behind
// contact_query.inl; PhysicsSystem::setupPhysicsStepTasks hands the host stub to
// the runtime (mwhip_set_shape_kernel), which owns the plans and launches it.
//
// One launch serves up to MWHIP_MAX_STEP_SHAPES queries.  A workgroup is 256
// threads = 4 wavefronts.  A work item is a BUNDLE of G shapes that share a
// world; wavefronts stride over the bundles of all plans.  Per bundle:
//   * world and count are read and checked (BAD_WORLD, SKIPPED), then
//     WorldBodies::fill, as the step (UNSORTED where the step raises an error);
//   * every shape's inputs are checked (BAD_SHAPE) and its status and a count
//     of 0 written;
//   * the (shape g, body k) pairs, row-major over g then k, 64 per round, a pair
//     per lane: the lane reads the body (current pose) and the shape's inputs,
//     drops the pair if the body is the shape's excluded entity, and runs
//     setupPair's own box test for every primitive pair c = shapePrim *
//     body_num_prims + bodyPrim, the shape as `a`: a bit per primitive pair.
//     The shape's Loc is Loc::none(), which names no row: setupPair and the
//     narrowphase only carry it into ContactConstraint::ref / alt, and
//     storeHit reads the Entity of the side that is valid.  No tree is walked;
//   * survivors go in enumeration order to the wavefront's list in LDS;
//     whenever 64 wait there, and at the end, the narrowphase runs on a chunk,
//     exactly as contactq::collideChunk does: collidePairLane in lanePolyRows
//     rounds, hullHullWave pair after pair, collidePairStored for polygons that
//     outgrow LDS -- through THIS WAVEFRONT's slot of the executor's shape
//     scratch (two wavefronts of a launch may be in the same world, so the
//     world's slot of PhysicsScratch::worldHullScratch will not do).
//     MWHIP_SHAPES_PLAIN: every survivor through collidePairStored, one lane at
//     a time -- the definition itself;
//   * accepted lanes are ranked PER SHAPE.  A chunk holds ascending shapes, and
//     only its first shape can have hits from earlier chunks (the carry, a
//     wavefront-uniform pair): dst = carry (for that shape) + rank among the
//     accepted lanes of the same shape, stored only where dst < max_hits.  The
//     last listed lane of every shape of the chunk writes that shape's count;
//   * behind a fence the wavefront reads status and count of its shapes back,
//     fills every shape's tail and zeroes the count of a shape that is not OK.
// Every store index is below its buffer's length: a shape is below S, a slot
// below max_hits, a list index below listCap, the scratch slot below
// scratch_waves.  No atomics, no spin-waits, no workgroup barrier, no workgroup
// waits for another; plain vector stores.  No sticky error flag is raised.

namespace shapeq {

inline constexpr uint32_t listCap = 128;

// per wavefront: the step's narrowphase scratch and the list of the primitive
// pairs whose boxes intersect and that wait for the narrowphase
struct alignas(16) QueryScratch {
    WaveScratch narrow;
    uint32_t shape[listCap];    // g, the shape in the bundle
    uint32_t body[listCap];     // k, the body in the world
    uint32_t primS[listCap];    // primitive of the shape's object, of the body's
    uint32_t primB[listCap];
};

// one shape's inputs
struct ShapeIn {
    PrimitiveTransform txfm;
    Entity exclude;
    int32_t object;
    bool ok;                // finite pose, object in range
};

// what a bundle's query keeps across its phases (wavefront-uniform)
struct BundleQuery {
    Context *ctx;
    const ObjectManager *objMgr;
    const WorldBodies *bodies;
    const mwhip_shape_plan *plan;
    QueryScratch *scratch;
    char *hullSlot;         // this wavefront's slot of the executor's shape scratch
    uint32_t firstShape;    // bundle * G
    uint32_t maxHits;
    bool plain;
    uint32_t pending;       // pairs waiting in the list
    uint32_t carryShape;    // the last shape a chunk has stored hits of, ~0: none
    uint32_t carryCount;    // ... and how many so far
};

__device__ inline ShapeIn readShape(const mwhip_shape_plan *plan, uint32_t s)
{
    ShapeIn in;
    const float *p = plan->position + (uint64_t)s * 3ull;
    const float *r = plan->rotation + (uint64_t)s * 4ull;
    const float *c = plan->scale + (uint64_t)s * 3ull;
    in.txfm = PrimitiveTransform {
        Vector3 { p[0], p[1], p[2] }, Quat { r[0], r[1], r[2], r[3] },
        Diag3x3 { c[0], c[1], c[2] },
    };
    in.object = plan->object[s];
    const uint32_t *e = (const uint32_t *)(plan->exclude_src +
                                           (uint64_t)s * plan->exclude_stride);
    in.exclude = Entity { e[0], (int32_t)e[1] };
    bool finite = true;
#pragma unroll
    for (int32_t i = 0; i < 3; i++) {
        finite = finite && treeq::finiteBits(p[i]) && treeq::finiteBits(c[i]);
    }
#pragma unroll
    for (int32_t i = 0; i < 4; i++) {
        finite = finite && treeq::finiteBits(r[i]);
    }
    in.ok = finite && in.object >= 0 && (uint32_t)in.object < plan->num_objects;
    return in;
}

__device__ inline PrimitiveTransform bodyTransform(Context &ctx, Loc loc)
{
    return PrimitiveTransform {
        ctx.getDirect<base::Position>(RGDCols::Position, loc),
        ctx.getDirect<base::Rotation>(RGDCols::Rotation, loc),
        Diag3x3(ctx.getDirect<base::Scale>(RGDCols::Scale, loc)),
    };
}

// the shape is `a`, under a Loc that names no row
__device__ inline PairSetup pairOf(const BundleQuery &q, Loc body_loc, uint32_t s_prim_base,
                                   uint32_t b_prim_base, uint32_t s_prim, uint32_t b_prim,
                                   const PrimitiveTransform &s_txfm,
                                   const PrimitiveTransform &b_txfm)
{
    return setupPair(*q.objMgr, Loc::none(), body_loc, s_prim_base + s_prim,
                     b_prim_base + b_prim, s_txfm, b_txfm);
}

// the pair in list slot `slot` (< pending), as setupPair orders it
__device__ inline PairSetup listedPair(const BundleQuery &q, uint32_t slot)
{
    const QueryScratch *s = q.scratch;
    const ShapeIn in = readShape(q.plan, q.firstShape + s->shape[slot]);
    const Loc b_loc = q.bodies->loc((int32_t)s->body[slot]);
    const base::ObjectID b_obj = q.ctx->getDirect<base::ObjectID>(RGDCols::ObjectID, b_loc);
    return pairOf(q, b_loc, q.objMgr->rigidBodyPrimitiveOffsets[in.object],
                  q.objMgr->rigidBodyPrimitiveOffsets[b_obj.idx], s->primS[slot],
                  s->primB[slot], in.txfm, bodyTransform(*q.ctx, b_loc));
}

// (out of line: the generic routine is large and almost never taken by the
// cooperative mapping; bit 0: a contact was written, bit 1: unsupported)
__device__ __attribute__((noinline)) inline uint32_t
collideStoredOutOfLine(const PairSetup &pair, char *hull_slot, ContactConstraint *out)
{
    geo::Plane *tmp_faces = (geo::Plane *)hull_slot;
    static_assert(PhysicsScratch::hullScratchBytes >=
        MADRONA_PHYS_MAX_HULL_ELEMS * (sizeof(geo::Plane) + sizeof(math::Vector3)));
    math::Vector3 *tmp_vertices = (math::Vector3 *)(tmp_faces + MADRONA_PHYS_MAX_HULL_ELEMS);
    bool unsupported = false;
    const bool found = collidePairStored(pair, tmp_vertices, tmp_faces,
        MADRONA_PHYS_MAX_HULL_ELEMS, out, &unsupported);
    return (found ? 1u : 0u) | (unsupported ? 2u : 0u);
}

// (s < S, dst < max_hits: slot < S x K <= 2^31 - 1)
__device__ inline void storeHit(const BundleQuery &q, uint32_t s, uint32_t dst,
                                const ContactConstraint &contact)
{
    const mwhip_shape_plan *plan = q.plan;
    const uint64_t slot = (uint64_t)s * q.maxHits + dst;
    // the side that is a row: the shape's Loc is never dereferenced
    const bool shape_is_ref = !contact.ref.valid();
    const Entity hit = q.ctx->getDirect<Entity>(0, shape_is_ref ? contact.alt : contact.ref);
    uint32_t *e = plan->hits + slot * 2ull;
    e[0] = hit.gen;
    e[1] = (uint32_t)hit.id;
    plan->shape_is_ref[slot] = shape_is_ref ? 1 : 0;
    queryst::storeManifold(plan->num_points, plan->normal, plan->points, slot, contact);
}

__device__ inline void storeNoHit(const BundleQuery &q, uint32_t s, uint32_t dst)
{
    const mwhip_shape_plan *plan = q.plan;
    const uint64_t slot = (uint64_t)s * q.maxHits + dst;
    const Entity none = Entity::none();
    uint32_t *e = plan->hits + slot * 2ull;
    e[0] = none.gen;
    e[1] = (uint32_t)none.id;
    plan->shape_is_ref[slot] = 0;
    queryst::storeNoManifold(plan->num_points, plan->normal, plan->points, slot);
}

// The narrowphase on list slots [0, n), n <= 64, a pair per lane, then the
// list moves down by n.  contactq::collideChunk with the ranking per shape.
__device__ inline void collideChunk(BundleQuery &q, uint32_t lane, uint32_t n)
{
    QueryScratch *scratch = q.scratch;
    ContactConstraint contact;
    bool has_contact = false;
    bool too_big = false;
    bool unsupported = false;

    // (every listed pair passed setupPair's box test)
    uint32_t kind = 0;      // 1: this lane alone, 2: whole wave, 3: stored
    uint32_t g = 0xFFFFFFFFu;
    PairSetup pair;
    if (lane < n) {
        g = scratch->shape[lane];
        pair = listedPair(q, lane);
        kind = q.plain ? 3u : pair.test == NarrowphaseTest::HullHull ? 2u : 1u;
    }

    // lanes on their own, in rounds of lanePolyRows scratch rows
    const uint64_t solo = __builtin_amdgcn_ballot_w64(kind == 1u);
    const uint32_t solo_rank = wave::rankInBallot(solo);
    const uint32_t solo_count = (uint32_t)__builtin_popcountll(solo);
    for (uint32_t first = 0; first < solo_count; first += lanePolyRows) {
        if (kind == 1u && solo_rank >= first && solo_rank < first + lanePolyRows) {
            has_contact = collidePairLane(pair,
                scratch->narrow.lanePoly + (solo_rank - first) * lanePolyDwords,
                &contact, &too_big, &unsupported);
        }
    }

    // hull-hull pairs: one after the other, SAT loops over the lanes
    uint64_t hull_pairs = __builtin_amdgcn_ballot_w64(kind == 2u);
    while (hull_pairs != 0) {
        const uint32_t src = (uint32_t)__builtin_ctzll(hull_pairs);
        hull_pairs &= hull_pairs - 1;

        const PairSetup shared_pair = listedPair(q, src);
        ContactConstraint shared_contact;
        bool shared_too_big = false;
        const bool found = hullHullWave(lane, shared_pair, &scratch->narrow.hull,
            &shared_contact, &shared_too_big);
        if (lane == src) {
            contact = shared_contact;
            has_contact = found;
            too_big = shared_too_big;
        }
    }

    // polygons larger than the LDS scratch, and every pair of the plain
    // mapping: the generic routine, one lane at a time through the wavefront's
    // scratch in HBM
    uint64_t stored_pairs = __builtin_amdgcn_ballot_w64(too_big || kind == 3u);
    while (stored_pairs != 0) {
        const uint32_t src = (uint32_t)__builtin_ctzll(stored_pairs);
        stored_pairs &= stored_pairs - 1;
        if (lane == src) {
            const uint32_t outcome = collideStoredOutOfLine(pair, q.hullSlot, &contact);
            has_contact = (outcome & 1u) != 0u;
            unsupported = unsupported || (outcome & 2u) != 0u;
        }
        wave::phaseFence();
    }

    // ---- rank per shape: the lanes of a shape are consecutive ----
    const uint32_t g_before = (uint32_t)__shfl_up((int32_t)g, 1u, 64);
    const uint32_t g_after = (uint32_t)__shfl_down((int32_t)g, 1u, 64);
    const bool listed = lane < n;
    const bool run_head = listed && (lane == 0u || g_before != g);
    const bool run_tail = listed && (lane + 1u == n || g_after != g);
    const uint64_t heads = __builtin_amdgcn_ballot_w64(run_head);
    const uint64_t tails = __builtin_amdgcn_ballot_w64(run_tail);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(has_contact);
    const uint64_t bad = __builtin_amdgcn_ballot_w64(unsupported);
    if (listed) {
        // [my_head, my_tail]: the lanes of this lane's shape
        const uint64_t upto = lane == 63u ? ~0ull : (1ull << (lane + 1u)) - 1ull;
        const uint32_t my_head = 63u - (uint32_t)__builtin_clzll(heads & upto);
        const uint32_t my_tail = (uint32_t)__builtin_ctzll(tails & ~(upto >> 1));
        const uint64_t run = (my_tail == 63u ? ~0ull : (1ull << (my_tail + 1u)) - 1ull) &
            ~((1ull << my_head) - 1ull);
        const uint32_t before = g == q.carryShape ? q.carryCount : 0u;
        const uint32_t dst = before +
            (uint32_t)__builtin_popcountll(mask & run & ((1ull << lane) - 1ull));
        const uint32_t s = q.firstShape + g;
        if (has_contact && dst < q.maxHits) {
            storeHit(q, s, dst, contact);
        }
        if (lane == my_tail) {
            q.plan->count[s] = (int32_t)(before + (uint32_t)__builtin_popcountll(mask & run));
            if ((bad & run) != 0ull) {
                q.plan->status[s] = MWHIP_SHAPES_UNSUPPORTED;
            }
        }
    }
    // the carry: the chunk's last shape and its hits so far
    {
        const uint32_t last = n - 1u;
        const uint32_t g_last = (uint32_t)__shfl((int32_t)g, (int)last, 64);
        const uint64_t upto_last = last == 63u ? ~0ull : (1ull << (last + 1u)) - 1ull;
        const uint32_t head_last = 63u - (uint32_t)__builtin_clzll(heads & upto_last);
        const uint64_t run_last = upto_last & ~((1ull << head_last) - 1ull);
        const uint32_t before = g_last == q.carryShape ? q.carryCount : 0u;
        q.carryCount = before + (uint32_t)__builtin_popcountll(mask & run_last);
        q.carryShape = g_last;
    }

    // what waits behind the chunk moves to the front (pending <= listCap = 2 x
    // 64: at most one slot per lane)
    const uint32_t from = n + lane;
    const bool moves = from < q.pending;
    uint32_t moved[4] { 0, 0, 0, 0 };
    if (moves) {
        moved[0] = scratch->shape[from];
        moved[1] = scratch->body[from];
        moved[2] = scratch->primS[from];
        moved[3] = scratch->primB[from];
    }
    wave::phaseFence();
    if (moves) {
        scratch->shape[lane] = moved[0];
        scratch->body[lane] = moved[1];
        scratch->primS[lane] = moved[2];
        scratch->primB[lane] = moved[3];
    }
    q.pending -= n;
    wave::phaseFence();
}

__device__ inline void collideFullChunks(BundleQuery &q, uint32_t lane)
{
    while (q.pending >= 64u) {
        collideChunk(q, lane, 64u);
    }
}

// one bundle of one query, by one wavefront
__device__ inline void shapeBundle(const mwhip_shape_plan *plan, uint32_t bundle, uint32_t lane,
                                   QueryScratch *scratch, char *hull_slot)
{
    EcsState *S = (EcsState *)plan->state;
    StateManager *state_mgr = static_cast<StateManager *>(S);
    PhysicsScratch *ps = detail::scratch(S);
    const uint32_t max_hits = plan->max_hits;
    const uint32_t G = plan->shapes_per_bundle;
    const uint32_t first_shape = bundle * G;

    // ---- world, then count (every lane reads the same words) ----
    int32_t status = MWHIP_SHAPES_OK;
    int32_t world;
    const uint32_t per_world = plan->bundles_per_world;
    if (per_world != 0u) {
        world = (int32_t)(bundle / per_world);
    } else {
        world = *(const int32_t *)(plan->world_src + (uint64_t)bundle * plan->world_stride);
    }
    if (world < 0 || world >= S->numWorlds) {
        status = MWHIP_SHAPES_BAD_WORLD;
        world = 0;
    } else if (plan->count_src != nullptr && per_world != 0u &&
               (int32_t)(bundle % per_world) >=
                   *(const int32_t *)(plan->count_src +
                                      (uint64_t)(uint32_t)world * plan->count_stride)) {
        status = MWHIP_SHAPES_SKIPPED;
    }
    world = __builtin_amdgcn_readfirstlane(world);
    status = __builtin_amdgcn_readfirstlane(status);

    Context ctx = TaskGraph::makeContext<Context>(state_mgr, WorldID { world });
    WorldBodies bodies;
    if (status == MWHIP_SHAPES_OK && !bodies.fill(S, ps, world)) {
        status = MWHIP_SHAPES_UNSORTED;
    }

    BundleQuery q;
    q.ctx = &ctx;
    q.bodies = &bodies;
    q.plan = plan;
    q.scratch = scratch;
    q.hullSlot = hull_slot;
    q.firstShape = first_shape;
    q.maxHits = max_hits;
    q.plain = (plan->flags & MWHIP_SHAPES_PLAIN) != 0u;
    q.pending = 0;
    q.carryShape = 0xFFFFFFFFu;
    q.carryCount = 0;

    // ---- every shape's own check; status and a count of 0 ----
    for (uint32_t g = lane; g < G; g += 64u) {
        int32_t shape_status = status;
        if (status == MWHIP_SHAPES_OK && !readShape(plan, first_shape + g).ok) {
            shape_status = MWHIP_SHAPES_BAD_SHAPE;
        }
        plan->status[first_shape + g] = shape_status;
        plan->count[first_shape + g] = 0;
    }
    // (a chunk may store a shape's count and UNSUPPORTED behind these)
    wave::phaseFence();

    if (status == MWHIP_SHAPES_OK) {
        const ObjectManager &obj_mgr = *ctx.singleton<ObjectData>().mgr;
        q.objMgr = &obj_mgr;

        const uint32_t num_bodies = (uint32_t)bodies.count();
        const uint64_t num_pairs = (uint64_t)G * num_bodies;
        for (uint64_t base = 0; base < num_pairs; base += 64ull) {
            const uint64_t p = base + lane;
            const bool valid = p < num_pairs;

            // ---- the lane's (shape, body): how many primitive pairs ----
            uint32_t g = 0, k = 0, prims_b = 1, num_prim_pairs = 0;
            uint32_t s_prim_base = 0, b_prim_base = 0;
            Loc b_loc { 0, 0 };
            ShapeIn in;
            in.ok = false;
            if (valid) {
                g = (uint32_t)(p / num_bodies);
                k = (uint32_t)(p % num_bodies);
                in = readShape(plan, first_shape + g);
            }
            if (in.ok) {
                b_loc = bodies.loc((int32_t)k);
                const Entity b_e = ctx.getDirect<Entity>(0, b_loc);
                if (b_e != in.exclude) {
                    const base::ObjectID b_obj =
                        ctx.getDirect<base::ObjectID>(RGDCols::ObjectID, b_loc);
                    s_prim_base = obj_mgr.rigidBodyPrimitiveOffsets[in.object];
                    b_prim_base = obj_mgr.rigidBodyPrimitiveOffsets[b_obj.idx];
                    prims_b = obj_mgr.rigidBodyPrimitiveCounts[b_obj.idx];
                    num_prim_pairs = obj_mgr.rigidBodyPrimitiveCounts[in.object] * prims_b;
                    if (prims_b == 0u) {
                        prims_b = 1;
                    }
                }
            }

            const uint32_t most = wave::maxReduce(num_prim_pairs);
            if (most <= 64u) {
                // ---- a bit per primitive pair whose boxes intersect ----
                uint64_t overlap = 0;
                if (num_prim_pairs != 0u) {
                    const PrimitiveTransform b_txfm = bodyTransform(ctx, b_loc);
                    for (uint32_t c = 0; c < num_prim_pairs; c++) {
                        if (pairOf(q, b_loc, s_prim_base, b_prim_base, c / prims_b, c % prims_b,
                                   in.txfm, b_txfm).aabbOverlap) {
                            overlap |= 1ull << c;
                        }
                    }
                }
                uint32_t round_total;
                const uint32_t first = wave::exclusiveScan(
                    (uint32_t)__builtin_popcountll(overlap), lane, &round_total);

                // ---- into the list in enumeration order, as much as fits ----
                uint32_t done = 0;
                while (done < round_total) {
                    const uint32_t room = listCap - q.pending;
                    const uint32_t take = round_total - done < room ? round_total - done : room;
                    uint64_t left = overlap;
                    uint32_t idx = first;
                    while (left != 0ull) {
                        const uint32_t c = (uint32_t)__builtin_ctzll(left);
                        left &= left - 1ull;
                        if (idx >= done && idx < done + take) {
                            // (pending + take <= listCap)
                            const uint32_t slot = q.pending + (idx - done);
                            scratch->shape[slot] = g;
                            scratch->body[slot] = k;
                            scratch->primS[slot] = c / prims_b;
                            scratch->primB[slot] = c % prims_b;
                        }
                        idx += 1u;
                    }
                    q.pending += take;
                    done += take;
                    wave::phaseFence();
                    collideFullChunks(q, lane);
                }
            } else {
                // ---- a (shape, body) with more than 64 primitive pairs: the
                // round pair by pair, 64 primitive pairs at a time ----
                for (uint32_t t = 0; t < 64u; t++) {
                    const uint32_t pairs_t = (uint32_t)__shfl((int32_t)num_prim_pairs, (int)t, 64);
                    if (pairs_t == 0u) {
                        continue;
                    }
                    const uint32_t g_t = (uint32_t)__shfl((int32_t)g, (int)t, 64);
                    const uint32_t k_t = (uint32_t)__shfl((int32_t)k, (int)t, 64);
                    const uint32_t prims_b_t = (uint32_t)__shfl((int32_t)prims_b, (int)t, 64);
                    const uint32_t s_base_t = (uint32_t)__shfl((int32_t)s_prim_base, (int)t, 64);
                    const uint32_t b_base_t = (uint32_t)__shfl((int32_t)b_prim_base, (int)t, 64);
                    const Loc b_loc_t = bodies.loc((int32_t)k_t);
                    const ShapeIn in_t = readShape(plan, first_shape + g_t);
                    const PrimitiveTransform b_txfm = bodyTransform(ctx, b_loc_t);
                    for (uint32_t c_base = 0; c_base < pairs_t; c_base += 64u) {
                        const uint32_t c = c_base + lane;
                        const bool overlaps = c < pairs_t &&
                            pairOf(q, b_loc_t, s_base_t, b_base_t, c / prims_b_t, c % prims_b_t,
                                   in_t.txfm, b_txfm).aabbOverlap;
                        const uint64_t mask = __builtin_amdgcn_ballot_w64(overlaps);
                        if (overlaps) {
                            // (pending < 64 here and at most 64 join: < listCap)
                            const uint32_t slot = q.pending + wave::rankInBallot(mask);
                            scratch->shape[slot] = g_t;
                            scratch->body[slot] = k_t;
                            scratch->primS[slot] = c / prims_b_t;
                            scratch->primB[slot] = c % prims_b_t;
                        }
                        q.pending += (uint32_t)__builtin_popcountll(mask);
                        wave::phaseFence();
                        collideFullChunks(q, lane);
                    }
                }
            }
        }
        if (q.pending != 0u) {
            collideChunk(q, lane, q.pending);
        }
    }

    // ---- what no hit took: status and count of every shape read back behind
    // the chunks' stores (a shape that turned out UNSUPPORTED loses what its
    // first chunks stored) ----
    wave::phaseFence();
    const uint64_t num_slots = (uint64_t)G * max_hits;
    for (uint64_t i = lane; i < num_slots; i += 64ull) {
        const uint32_t g = (uint32_t)(i / max_hits);
        const uint32_t k = (uint32_t)(i % max_hits);
        const uint32_t s = first_shape + g;
        const uint32_t count = plan->status[s] == MWHIP_SHAPES_OK ? (uint32_t)plan->count[s] : 0u;
        if (k >= count) {
            storeNoHit(q, s, k);
        }
    }
    wave::phaseFence();
    for (uint32_t g = lane; g < G; g += 64u) {
        if (plan->status[first_shape + g] != MWHIP_SHAPES_OK) {
            plan->count[first_shape + g] = 0;
        }
    }
    // (the next bundle of this wavefront reuses the scratch)
    wave::phaseFence();
}

}

// (wavefronts per SIMD the register allocator aims at: DESIGN.md section 39)
#ifndef MADRONA_SHAPE_WAVES_PER_EU
#define MADRONA_SHAPE_WAVES_PER_EU 1
#endif
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(MADRONA_SHAPE_WAVES_PER_EU)))
shapeQueryKernel(mwhip_shape_args args)
{
    const uint32_t lane = wave::laneID();
    const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    __shared__ shapeq::QueryScratch block_scratch[4];
    shapeq::QueryScratch *scratch = &block_scratch[wave_in_block];

    const uint32_t num_plans = args.num_plans < MWHIP_MAX_STEP_SHAPES ?
        args.num_plans : MWHIP_MAX_STEP_SHAPES;
    const uint32_t wave_global = blockIdx.x * 4u + wave_in_block;
    uint32_t first_item = 0;
    for (uint32_t p = 0; p < num_plans; p++) {
        // (constant indices: the arguments stay in scalar registers)
        const mwhip_shape_plan *plan = args.plans[0];
        uint32_t items = args.items[0];
#pragma unroll
        for (uint32_t other = 1; other < MWHIP_MAX_STEP_SHAPES; other++) {
            if (p == other) {
                plan = args.plans[other];
                items = args.items[other];
            }
        }
        // (a wavefront without a scratch slot serves nothing: the runtime's
        // grid never has one)
        if (wave_global >= plan->scratch_waves) {
            return;
        }
        char *hull_slot = plan->scratch + (size_t)wave_global * plan->scratch_stride;
        const uint32_t bundles = items < plan->num_bundles ? items : plan->num_bundles;
        // wavefronts stride over the bundles of all plans, plan after plan
        const uint32_t stride = gridDim.x * 4u;
        uint32_t bundle = (wave_global + stride - first_item % stride) % stride;
        for (; bundle < bundles; bundle += stride) {
            shapeq::shapeBundle(plan, bundle, lane, scratch, hull_slot);
        }
        first_item += items;
    }
}
