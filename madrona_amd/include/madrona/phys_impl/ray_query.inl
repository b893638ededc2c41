// Ray queries (mwhip_rays_*, include/mwhip.h): tensors of
// rays cast through the worlds' broadphase BVHs.  Included by physics.inl inside
// madrona::phys::kernels, so the kernel is part of every simulator library that
// has a broadphase: BVH::traceRayShared and its LDS scratch live there, and
// PhysicsSystem::setupBroadphaseTasks hands the host stub to the runtime
// (mwhip_set_ray_kernel), which owns the plans and launches it.
//
// One launch serves up to MWHIP_MAX_STEP_RAYS queries.  A workgroup is 256
// threads = 4 wavefronts = 8 groups of 32 lanes, the shape rayGroupScratch()
// accepts (39 KB of LDS per workgroup: 4 workgroups, 16 wavefronts, per CU).  A
// work item is a wavefront, i.e. two groups, of ONE query; wavefronts stride
// over the items.
//   groups_per_fan > 0 (R >= 8): group g of the query holds rays
//       (g % groups_per_fan) * 32 + lane of fan g / groups_per_fan and goes
//       through traceRayShared: the ray-independent half of a leaf test once
//       per leaf and group;
//   groups_per_fan == 0 (R < 8): ray g * 32 + lane, whatever its fan, through
//       plain traceRay.
// traceRayShared gives the bits of traceRay, so do the two mappings.
// The leader of a ray's fan in its group (lane 0 of the group; the lane itself
// when rays are packed) reads and checks what the fan has -- world, count,
// origin, in that order, nothing behind a check that failed -- and the group's
// lanes take the result from it with a cross-lane read.  Each lane then checks
// its own direction and t_max.  Only lanes whose status is still 0 go to a
// tree, that of their (checked) world, found as ctx.singleton<BVH>() finds it.
// A ray sees the tree as the last broadphase pass left it (broadphase.hpp,
// BVH::traceRay's precondition); spheres are transparent (traceRayIntoLeaf).
// A world whose tree was never built (numNodes() == 0) gives MISS without the
// tree being touched.  Every loop is traceRay's own: over the leaves of a built
// tree, or, while a rebuild of a built tree is pending, the stack walk over its
// (old, valid) nodes that the simulators' own ray nodes take.  No atomics,
// no spin-waits, no workgroup barrier (the groups only use wave barriers), no
// workgroup waits for another; plain vector stores.

namespace rayq {

using treeq::finiteBits;
using treeq::nanBits;

// one wavefront: groups 2 * item and 2 * item + 1 of one query
__device__ inline void rayWave(const mwhip_ray_plan *plan, uint32_t item, uint32_t lane,
                               broadphase::BVH::RayGroupScratch *scratch)
{
    using math::Vector3;
    using broadphase::BVH;

    EcsState *S = (EcsState *)plan->state;
    const uint32_t num_fans = plan->num_fans;
    const uint32_t rays_per_fan = plan->rays_per_fan;
    const uint32_t fans_per_world = plan->fans_per_world;
    const uint32_t groups_per_fan = plan->groups_per_fan;
    const uint32_t num_rays = num_fans * rays_per_fan;      // <= 2^31 - 1 (create)

    const uint64_t group = (uint64_t)item * 2ull + (lane >> 5);
    const uint32_t group_lane = lane & 31u;

    bool valid;
    uint32_t fan = 0, ray = 0;
    uint32_t leader = lane;
    if (groups_per_fan != 0u) {
        const uint64_t f = group / groups_per_fan;
        const uint32_t r = (uint32_t)(group % groups_per_fan) * 32u + group_lane;
        valid = f < (uint64_t)num_fans && r < rays_per_fan;
        if (valid) {
            fan = (uint32_t)f;
            ray = fan * rays_per_fan + r;
        }
        leader = lane & ~31u;       // (r = 32 * chunk < R: valid whenever the fan is)
    } else {
        const uint64_t i = group * 32ull + group_lane;
        valid = i < (uint64_t)num_rays;
        if (valid) {
            ray = (uint32_t)i;
            fan = ray / rays_per_fan;
        }
    }

    // ---- per fan, by its leader ----
    int32_t status = MWHIP_RAYS_MISS;
    int32_t world = 0;
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (valid && lane == leader) {
        const treeq::GroupHead head = treeq::readGroupHead(
            plan->world_src, plan->world_stride, plan->count_src, plan->count_stride,
            plan->origin_src, plan->origin_stride, fans_per_world, fan, S);
        status = head.code == treeq::HeadCode::BadWorld ? MWHIP_RAYS_BAD_WORLD :
            head.code == treeq::HeadCode::Skipped ? MWHIP_RAYS_SKIPPED :
            head.code == treeq::HeadCode::BadPoint ? MWHIP_RAYS_BAD_RAY : MWHIP_RAYS_MISS;
        world = head.world;
        ox = head.x;
        oy = head.y;
        oz = head.z;
    }
    // (every lane of the wavefront takes part in the cross-lane reads)
    status = __shfl(status, (int)leader, 64);
    world = __shfl(world, (int)leader, 64);
    ox = __shfl(ox, (int)leader, 64);
    oy = __shfl(oy, (int)leader, 64);
    oz = __shfl(oz, (int)leader, 64);

    // ---- per ray ----
    float dx = 0.f, dy = 0.f, dz = 0.f, t_max = 0.f;
    if (valid && status == MWHIP_RAYS_MISS) {
        const float *d = plan->dir + (uint64_t)ray * 3ull;
        dx = d[0];
        dy = d[1];
        dz = d[2];
        t_max = plan->t_max[ray];
        if (!finiteBits(dx) || !finiteBits(dy) || !finiteBits(dz) ||
                (dx == 0.f && dy == 0.f && dz == 0.f) || nanBits(t_max)) {
            status = MWHIP_RAYS_BAD_RAY;
        }
    }

    float hit_t = 0.f;
    Entity hit = Entity::none();
    Vector3 normal = Vector3::zero();
    if (valid && status == MWHIP_RAYS_MISS) {
        BVH *trees = static_cast<StateManager *>(S)->getSingletonColumn<BVH>();
        BVH &bvh = trees[world];
        const Vector3 o { ox, oy, oz };
        const Vector3 d { dx, dy, dz };
        float t = 0.f;
        Vector3 n = Vector3::zero();
        Entity e = Entity::none();
        // A tree that no broadphase pass has built yet (numNodes() == 0: a
        // world before its first step, or restored to that state) has a
        // rebuild pending and node memory nobody wrote: the pending-rebuild
        // walk of traceRay must not see it.  Nothing is built, nothing is
        // met: MISS, the tree untouched.  (The lanes of a group share their
        // world, so a group enters the tracer together or not at all.)
        if (bvh.numNodes() != 0) {
            // (the mapping is the same for the whole wavefront)
            e = groups_per_fan != 0u ?
                bvh.traceRayShared(scratch, o, d, &t, &n, t_max) :
                bvh.traceRay(o, d, &t, &n, t_max);
        }
        if (e != Entity::none()) {
            status = MWHIP_RAYS_HIT;
            hit_t = t;
            hit = e;
            normal = n;
        }
    }

    if (valid) {
        plan->status[ray] = status;
        plan->hit_t[ray] = hit_t;
        uint32_t *h = plan->hit + (uint64_t)ray * 2ull;
        h[0] = hit.gen;
        h[1] = (uint32_t)hit.id;
        float *nrm = plan->normal + (uint64_t)ray * 3ull;
        nrm[0] = normal.x;
        nrm[1] = normal.y;
        nrm[2] = normal.z;
    }
}

}

__global__ void __launch_bounds__(256)
rayQueryKernel(mwhip_ray_args args)
{
    const uint32_t lane = wave::laneID();
    const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    broadphase::BVH::RayGroupScratch *scratch = broadphase::rayGroupScratch();

    uint32_t total = 0;
#pragma unroll
    for (uint32_t p = 0; p < MWHIP_MAX_STEP_RAYS; p++) {
        if (p < args.num_plans) total += args.items[p];
    }
    for (uint32_t item = blockIdx.x * 4u + wave_in_block; item < total;
         item += gridDim.x * 4u) {
        // the query this item belongs to (constant indices: the arguments stay
        // in scalar registers)
        const mwhip_ray_plan *plan = nullptr;
        uint32_t rel = item;
#pragma unroll
        for (uint32_t p = 0; p < MWHIP_MAX_STEP_RAYS; p++) {
            if (plan == nullptr && p < args.num_plans) {
                if (rel < args.items[p]) {
                    plan = args.plans[p];
                } else {
                    rel -= args.items[p];
                }
            }
        }
        if (plan != nullptr) {
            rayq::rayWave(plan, rel, lane, scratch);
        }
    }
}
