// Contact queries (mwhip_contacts_*, include/mwhip.h): per
// world the primitive pairs of its rigid bodies that touch, with the manifold
// the step's narrowphase builds for each, in the order (k_lo, k_hi, primitive
// pair).  Included by physics.inl inside madrona::phys::kernels behind
// box_query.inl, so the kernel is part of every simulator library that has a
// rigid-body step; PhysicsSystem::setupPhysicsStepTasks hands the host stub to
// the runtime (mwhip_set_contact_kernel), which owns the plans and launches it.
//
// One launch serves up to MWHIP_MAX_STEP_CONTACTS queries.  A workgroup is 256
// threads = 4 wavefronts.  A work item is a WORLD; wavefronts stride over the
// worlds and serve a world for one plan after the other (so that no two
// wavefronts of a launch are in the same world: its slot of
// PhysicsScratch::worldHullScratch has one user at a time).  Per world:
//   * WorldBodies::fill, as the step (UNSORTED where the step raises an error);
//   * the body pairs k_lo < k_hi, 64 per round, a pair per lane: the lane reads
//     both bodies (pose of the plan's mode), takes the one of lower entity id
//     as `a`, and runs setupPair's own box test for every primitive pair of the
//     two, in the order of the definition: a bit per primitive pair.  No test
//     coarser than that one is made, and no tree is walked: all pairs of a
//     world are n^2 / 2 box tests over 64 lanes, and the result is a function
//     of the tables alone (leaf boxes belong to other poses than the solver's
//     and go stale after a world write);
//   * the survivors of a round go, in enumeration order (a prefix sum over the
//     lanes' bit counts), to the wavefront's list in LDS.  Whenever 64 wait
//     there, and at the end, the narrowphase runs on a chunk -- full chunks, so
//     that the one-after-another hull-hull rounds are not spent on a few lanes,
//     and in order.  (A round in which some body pair has more than 64
//     primitive pairs is taken body pair by body pair, 64 primitive pairs at a
//     time, by ballot.)
//   * the narrowphase of a chunk is physicsStepKernel's (step_hbm.inl):
//     collidePairLane on lanePoly rows in rounds, hullHullWave on the
//     wavefront's HullScratch, one pair after the other, and for faces that
//     outgrow the LDS scratch collidePairStored, one lane at a time through the
//     world's slot of PhysicsScratch::worldHullScratch.  The same device
//     functions in a loop of the query's own: the step kernels are untouched.
//     MWHIP_CONTACTS_PLAIN: every survivor through collidePairStored, one lane
//     at a time through that slot -- the definition itself, and slow.
//   * accepted lanes are ranked by ballot: dst = running count + rank, stored
//     only where dst < max_contacts; the same wavefront then fills the tail
//     with Entity::none() and zeros and writes status and count.
// Every store index is below its buffer's length: a world is below num_worlds,
// a slot below max_contacts, a list index below listCap.  Every loop bound is
// read once.  No atomics, no spin-waits, no workgroup barrier, no workgroup
// waits for another; plain vector stores.  No sticky error flag is raised.

namespace contactq {

inline constexpr uint32_t listCap = 128;

// per wavefront: the step's narrowphase scratch and the list of the primitive
// pairs whose boxes intersect and that wait for the narrowphase
struct alignas(16) QueryScratch {
    WaveScratch narrow;
    uint32_t bodyA[listCap];    // index of body a in the world (lower entity id)
    uint32_t bodyB[listCap];
    uint32_t primA[listCap];    // primitive of a's object, of b's
    uint32_t primB[listCap];
};

// what a world's query keeps across its phases (wavefront-uniform)
struct WorldQuery {
    Context *ctx;
    const ObjectManager *objMgr;
    const WorldBodies *bodies;
    const mwhip_contact_plan *plan;
    QueryScratch *scratch;
    char *hullSlot;         // the world's slot of PhysicsScratch::worldHullScratch
    int32_t world;
    uint32_t maxContacts;
    bool solverPoses;
    bool plain;
    uint32_t pending;       // pairs waiting in the list
    uint32_t count;         // contacts found so far
    bool unsupported;
};

// the pose of the plan's mode, the current scale
__device__ inline PrimitiveTransform bodyTransform(Context &ctx, Loc loc, bool solver_poses)
{
    Vector3 pos = ctx.getDirect<base::Position>(RGDCols::Position, loc);
    Quat rot = ctx.getDirect<base::Rotation>(RGDCols::Rotation, loc);
    if (solver_poses) {
        const xpbd::PreSolvePositional solved = ctx.getDirect<xpbd::PreSolvePositional>(
            xpbd::XPBDCols::PreSolvePositional, loc);
        // (all zero: no step has integrated this body since it was created)
        const bool never = solved.q.w == 0.f && solved.q.x == 0.f && solved.q.y == 0.f &&
            solved.q.z == 0.f;
        if (!never) {
            pos = solved.x;
            rot = solved.q;
        }
    }
    return PrimitiveTransform {
        pos, rot, Diag3x3(ctx.getDirect<base::Scale>(RGDCols::Scale, loc)),
    };
}

__device__ inline PairSetup pairOf(const WorldQuery &q, Loc a_loc, Loc b_loc,
                                   uint32_t a_prim_base, uint32_t b_prim_base, uint32_t a_prim,
                                   uint32_t b_prim, const PrimitiveTransform &a_txfm,
                                   const PrimitiveTransform &b_txfm)
{
    return setupPair(*q.objMgr, a_loc, b_loc, a_prim_base + a_prim, b_prim_base + b_prim,
                     a_txfm, b_txfm);
}

// the pair in list slot `slot` (< pending), as setupPair orders it
__device__ inline PairSetup listedPair(const WorldQuery &q, uint32_t slot)
{
    const QueryScratch *s = q.scratch;
    const Loc a_loc = q.bodies->loc((int32_t)s->bodyA[slot]);
    const Loc b_loc = q.bodies->loc((int32_t)s->bodyB[slot]);
    const base::ObjectID a_obj = q.ctx->getDirect<base::ObjectID>(RGDCols::ObjectID, a_loc);
    const base::ObjectID b_obj = q.ctx->getDirect<base::ObjectID>(RGDCols::ObjectID, b_loc);
    return pairOf(q, a_loc, b_loc, q.objMgr->rigidBodyPrimitiveOffsets[a_obj.idx],
                  q.objMgr->rigidBodyPrimitiveOffsets[b_obj.idx], s->primA[slot],
                  s->primB[slot], bodyTransform(*q.ctx, a_loc, q.solverPoses),
                  bodyTransform(*q.ctx, b_loc, q.solverPoses));
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

__device__ inline void storeContact(const WorldQuery &q, uint32_t dst,
                                    const ContactConstraint &contact)
{
    const mwhip_contact_plan *plan = q.plan;
    // (world < num_worlds, dst < max_contacts: slot < W x K, W x K x 2 <= 2^31 - 1)
    const uint64_t slot = (uint64_t)q.world * q.maxContacts + dst;
    const Entity ref = q.ctx->getDirect<Entity>(0, contact.ref);
    const Entity alt = q.ctx->getDirect<Entity>(0, contact.alt);
    uint32_t *pair = plan->pairs + slot * 4ull;
    pair[0] = ref.gen;
    pair[1] = (uint32_t)ref.id;
    pair[2] = alt.gen;
    pair[3] = (uint32_t)alt.id;
    plan->num_points[slot] = contact.numPoints;
    float *normal = plan->normal + slot * 3ull;
    normal[0] = contact.normal.x;
    normal[1] = contact.normal.y;
    normal[2] = contact.normal.z;
    float *points = plan->points + slot * 16ull;
#pragma unroll
    for (int32_t i = 0; i < 4; i++) {
        // (the step leaves what it likes behind numPoints)
        const bool used = i < contact.numPoints;
        points[i * 4 + 0] = used ? contact.points[i].x : 0.f;
        points[i * 4 + 1] = used ? contact.points[i].y : 0.f;
        points[i * 4 + 2] = used ? contact.points[i].z : 0.f;
        points[i * 4 + 3] = used ? contact.points[i].w : 0.f;
    }
}

__device__ inline void storeNoContact(const WorldQuery &q, uint32_t dst)
{
    const mwhip_contact_plan *plan = q.plan;
    const uint64_t slot = (uint64_t)q.world * q.maxContacts + dst;
    const Entity none = Entity::none();
    uint32_t *pair = plan->pairs + slot * 4ull;
    pair[0] = none.gen;
    pair[1] = (uint32_t)none.id;
    pair[2] = none.gen;
    pair[3] = (uint32_t)none.id;
    plan->num_points[slot] = 0;
    float *normal = plan->normal + slot * 3ull;
    normal[0] = normal[1] = normal[2] = 0.f;
    float *points = plan->points + slot * 16ull;
#pragma unroll
    for (int32_t i = 0; i < 16; i++) {
        points[i] = 0.f;
    }
}

// The narrowphase on list slots [0, n), n <= 64, a pair per lane, then the
// list moves down by n.  The loop of physicsStepKernel (step_hbm.inl) on the
// list instead of the candidate array.
__device__ inline void collideChunk(WorldQuery &q, uint32_t lane, uint32_t n)
{
    QueryScratch *scratch = q.scratch;
    ContactConstraint contact;
    bool has_contact = false;
    bool too_big = false;
    bool unsupported = false;

    // (every listed pair passed setupPair's box test)
    uint32_t kind = 0;      // 1: this lane alone, 2: whole wave, 3: stored
    PairSetup pair;
    if (lane < n) {
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
    // mapping: the generic routine, one lane at a time through the world's
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
    q.unsupported = q.unsupported || __builtin_amdgcn_ballot_w64(unsupported) != 0ull;

    const uint64_t mask = __builtin_amdgcn_ballot_w64(has_contact);
    const uint32_t dst = q.count + wave::rankInBallot(mask);
    if (has_contact && dst < q.maxContacts) {
        storeContact(q, dst, contact);
    }
    q.count += (uint32_t)__builtin_popcountll(mask);

    // what waits behind the chunk moves to the front (pending <= listCap = 2 x
    // 64: at most one slot per lane)
    const uint32_t from = n + lane;
    const bool moves = from < q.pending;
    uint32_t moved[4] { 0, 0, 0, 0 };
    if (moves) {
        moved[0] = scratch->bodyA[from];
        moved[1] = scratch->bodyB[from];
        moved[2] = scratch->primA[from];
        moved[3] = scratch->primB[from];
    }
    wave::phaseFence();
    if (moves) {
        scratch->bodyA[lane] = moved[0];
        scratch->bodyB[lane] = moved[1];
        scratch->primA[lane] = moved[2];
        scratch->primB[lane] = moved[3];
    }
    q.pending -= n;
    wave::phaseFence();
}

__device__ inline void collideFullChunks(WorldQuery &q, uint32_t lane)
{
    while (q.pending >= 64u) {
        collideChunk(q, lane, 64u);
    }
}

// one world of one query, by one wavefront
__device__ inline void contactWorld(const mwhip_contact_plan *plan, int32_t world,
                                    uint32_t lane, QueryScratch *scratch)
{
    EcsState *S = (EcsState *)plan->state;
    StateManager *state_mgr = static_cast<StateManager *>(S);
    PhysicsScratch *ps = detail::scratch(S);
    const uint32_t max_contacts = plan->max_contacts;
    const uint32_t flags = plan->flags;

    int32_t status = MWHIP_CONTACTS_OK;
    const char *select_src = plan->select_src;
    if (select_src != nullptr &&
            *(const int32_t *)(select_src + (uint64_t)world * plan->select_stride) == 0) {
        status = MWHIP_CONTACTS_SKIPPED;
    }

    Context ctx = TaskGraph::makeContext<Context>(state_mgr, WorldID { world });
    WorldBodies bodies;
    if (status == MWHIP_CONTACTS_OK && !bodies.fill(S, ps, world)) {
        status = MWHIP_CONTACTS_UNSORTED;
    }

    WorldQuery q;
    q.ctx = &ctx;
    q.bodies = &bodies;
    q.plan = plan;
    q.scratch = scratch;
    q.world = world;
    q.maxContacts = max_contacts;
    q.solverPoses = (flags & MWHIP_CONTACTS_CURRENT_POSES) == 0u;
    q.plain = (flags & MWHIP_CONTACTS_PLAIN) != 0u;
    q.pending = 0;
    q.count = 0;
    q.unsupported = false;

    if (status == MWHIP_CONTACTS_OK) {
        const ObjectManager &obj_mgr = *ctx.singleton<ObjectData>().mgr;
        q.objMgr = &obj_mgr;
        q.hullSlot = ps->worldHullScratch + (size_t)world * PhysicsScratch::hullScratchBytes;

        const int32_t num_bodies = bodies.count();
        const int64_t num_body_pairs = (int64_t)num_bodies * (num_bodies - 1) / 2;
        // this lane's body pair of the round: (k_lo, k_lo + 1 + rest), row-major
        // over the upper triangle
        int32_t k_lo = 0;
        int64_t rest = (int64_t)lane;
        for (int64_t base = 0; base < num_body_pairs; base += 64) {
            while (k_lo < num_bodies - 1 && rest >= (int64_t)(num_bodies - 1 - k_lo)) {
                rest -= (int64_t)(num_bodies - 1 - k_lo);
                k_lo += 1;
            }
            const bool valid = k_lo < num_bodies - 1;

            // ---- the lane's body pair: which is a, how many primitive pairs ----
            uint32_t k_a = 0, k_b = 0, prims_b = 1, num_prim_pairs = 0;
            Loc a_loc { 0, 0 }, b_loc { 0, 0 };
            uint32_t a_prim_base = 0, b_prim_base = 0;
            if (valid) {
                const int32_t k_hi = k_lo + 1 + (int32_t)rest;
                const Loc lo_loc = bodies.loc(k_lo), hi_loc = bodies.loc(k_hi);
                const Entity lo_e = ctx.getDirect<Entity>(0, lo_loc);
                const Entity hi_e = ctx.getDirect<Entity>(0, hi_loc);
                const bool both_static =
                    ctx.getDirect<ResponseType>(RGDCols::ResponseType, lo_loc) ==
                        ResponseType::Static &&
                    ctx.getDirect<ResponseType>(RGDCols::ResponseType, hi_loc) ==
                        ResponseType::Static;
                // (forEachCandidate: the body of lower entity id owns the pair)
                const bool lo_is_a = lo_e.id < hi_e.id;
                k_a = (uint32_t)(lo_is_a ? k_lo : k_hi);
                k_b = (uint32_t)(lo_is_a ? k_hi : k_lo);
                a_loc = lo_is_a ? lo_loc : hi_loc;
                b_loc = lo_is_a ? hi_loc : lo_loc;
                if (!both_static) {
                    const base::ObjectID a_obj =
                        ctx.getDirect<base::ObjectID>(RGDCols::ObjectID, a_loc);
                    const base::ObjectID b_obj =
                        ctx.getDirect<base::ObjectID>(RGDCols::ObjectID, b_loc);
                    a_prim_base = obj_mgr.rigidBodyPrimitiveOffsets[a_obj.idx];
                    b_prim_base = obj_mgr.rigidBodyPrimitiveOffsets[b_obj.idx];
                    prims_b = obj_mgr.rigidBodyPrimitiveCounts[b_obj.idx];
                    num_prim_pairs = obj_mgr.rigidBodyPrimitiveCounts[a_obj.idx] * prims_b;
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
                    const PrimitiveTransform a_txfm = bodyTransform(ctx, a_loc, q.solverPoses);
                    const PrimitiveTransform b_txfm = bodyTransform(ctx, b_loc, q.solverPoses);
                    for (uint32_t c = 0; c < num_prim_pairs; c++) {
                        if (pairOf(q, a_loc, b_loc, a_prim_base, b_prim_base, c / prims_b,
                                   c % prims_b, a_txfm, b_txfm).aabbOverlap) {
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
                            scratch->bodyA[slot] = k_a;
                            scratch->bodyB[slot] = k_b;
                            scratch->primA[slot] = c / prims_b;
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
                // ---- a body pair with more than 64 primitive pairs: the round
                // body pair by body pair, 64 primitive pairs at a time ----
                for (uint32_t t = 0; t < 64u; t++) {
                    const uint32_t pairs_t = (uint32_t)__shfl((int32_t)num_prim_pairs, (int)t, 64);
                    if (pairs_t == 0u) {
                        continue;
                    }
                    const uint32_t k_a_t = (uint32_t)__shfl((int32_t)k_a, (int)t, 64);
                    const uint32_t k_b_t = (uint32_t)__shfl((int32_t)k_b, (int)t, 64);
                    const uint32_t prims_b_t = (uint32_t)__shfl((int32_t)prims_b, (int)t, 64);
                    const uint32_t a_base_t = (uint32_t)__shfl((int32_t)a_prim_base, (int)t, 64);
                    const uint32_t b_base_t = (uint32_t)__shfl((int32_t)b_prim_base, (int)t, 64);
                    const Loc a_loc_t = bodies.loc((int32_t)k_a_t);
                    const Loc b_loc_t = bodies.loc((int32_t)k_b_t);
                    const PrimitiveTransform a_txfm = bodyTransform(ctx, a_loc_t, q.solverPoses);
                    const PrimitiveTransform b_txfm = bodyTransform(ctx, b_loc_t, q.solverPoses);
                    for (uint32_t c_base = 0; c_base < pairs_t; c_base += 64u) {
                        const uint32_t c = c_base + lane;
                        const bool overlaps = c < pairs_t &&
                            pairOf(q, a_loc_t, b_loc_t, a_base_t, b_base_t, c / prims_b_t,
                                   c % prims_b_t, a_txfm, b_txfm).aabbOverlap;
                        const uint64_t mask = __builtin_amdgcn_ballot_w64(overlaps);
                        if (overlaps) {
                            // (pending < 64 here and at most 64 join: < listCap)
                            const uint32_t slot = q.pending + wave::rankInBallot(mask);
                            scratch->bodyA[slot] = k_a_t;
                            scratch->bodyB[slot] = k_b_t;
                            scratch->primA[slot] = c / prims_b_t;
                            scratch->primB[slot] = c % prims_b_t;
                        }
                        q.pending += (uint32_t)__builtin_popcountll(mask);
                        wave::phaseFence();
                        collideFullChunks(q, lane);
                    }
                }
            }
            rest += 64;
        }
        if (q.pending != 0u) {
            collideChunk(q, lane, q.pending);
        }
        if (q.unsupported) {
            status = MWHIP_CONTACTS_UNSUPPORTED;
        }
    }

    // ---- what no contact took, then status and count ----
    const uint32_t count = status == MWHIP_CONTACTS_OK ? q.count : 0u;
    // (behind the stores of the chunks: a world that turned out UNSUPPORTED
    // overwrites what its first chunks stored)
    wave::phaseFence();
    for (uint32_t k = (count < max_contacts ? count : max_contacts) + lane; k < max_contacts;
         k += 64u) {
        storeNoContact(q, k);
    }
    if (lane == 0u) {
        plan->status[world] = status;
        plan->count[world] = (int32_t)count;
    }
    // (the next plan of this wavefront reuses the scratch)
    wave::phaseFence();
}

}

// (wavefronts per SIMD the register allocator aims at; measured: DESIGN.md
// section 36)
#ifndef MADRONA_CONTACT_WAVES_PER_EU
#define MADRONA_CONTACT_WAVES_PER_EU 1
#endif
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(MADRONA_CONTACT_WAVES_PER_EU)))
contactQueryKernel(mwhip_contact_args args)
{
    const uint32_t lane = wave::laneID();
    const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    __shared__ contactq::QueryScratch block_scratch[4];
    contactq::QueryScratch *scratch = &block_scratch[wave_in_block];

    const uint32_t num_plans = args.num_plans < MWHIP_MAX_STEP_CONTACTS ?
        args.num_plans : MWHIP_MAX_STEP_CONTACTS;
    // (every plan of an executor has its number of worlds)
    const uint32_t num_worlds = num_plans != 0u ? args.items[0] : 0u;
    for (uint32_t world = blockIdx.x * 4u + wave_in_block; world < num_worlds;
         world += gridDim.x * 4u) {
        for (uint32_t p = 0; p < num_plans; p++) {
            // (constant indices: the arguments stay in scalar registers)
            const mwhip_contact_plan *plan = args.plans[0];
#pragma unroll
            for (uint32_t other = 1; other < MWHIP_MAX_STEP_CONTACTS; other++) {
                if (p == other) {
                    plan = args.plans[other];
                }
            }
            if (world < plan->num_worlds) {
                contactq::contactWorld(plan, (int32_t)world, lane, scratch);
            }
        }
    }
}
