// libmadrona_hip.so -- ray queries: N = F x R rays, F fans of R rays that share an
// origin and a world, cast through the worlds' broadphase BVHs (mwhip_rays_*,
// include/mwhip.h; madrona_amd/ray_ref.py is the definition).
//
// This file is the host side only.  The kernel, rayQueryKernel, is compiled
// into the simulator's code object (include/madrona/phys_impl/ray_query.inl),
// where BVH::traceRayShared and its LDS scratch live;
// PhysicsSystem::setupBroadphaseTasks registers its host stub
// (mwhip_set_ray_kernel) and the runtime launches it, as it launches a
// simulator's ParallelFor group kernel.  What the two code objects share is the
// POD pair mwhip_ray_plan / mwhip_ray_args of mwhip.h.
// A query owns a device-resident plan and ONE allocation with its owned inputs
// (world and origin unless a source was given; direction and t_max always) and
// its outputs (hit_t, hit, normal, status), 256-byte aligned each.  Sources are
// read on the device when the kernel runs, as a gather's.  What a box query has
// too is in tree_query.hpp.
#include "tree_query.hpp"

namespace {

constexpr uint32_t kRayThreads = 256;
constexpr uint32_t kRayWaves = kRayThreads / 64u;

}

struct mwhip_rays_rec : TreeQueryRec<mwhip_ray_plan, MWHIP_RAYS_NUM_BUFS> {
    uint32_t numFans = 0;
    uint32_t raysPerFan = 0;
    uint32_t numRays = 0;
};

namespace {

mwhip_rays_rec *findRays(mwhip_exec *exec, uint64_t handle)
{
    return findObject(exec != nullptr ? &exec->rays : nullptr, handle);
}

// (four workgroups of 39 KB of LDS fit a CU; wavefronts stride over the items)
dim3 rayGrid(mwhip_exec *exec, uint32_t items)
{
    return waveGrid(exec, items, kRayWaves, 8u);
}

int queueRays(mwhip_exec *exec, mwhip_rays_rec &rays)
{
    return queueBatch(exec, exec->rayKernel, rayGrid(exec, rays.items), kRayThreads,
                      singleBatch<mwhip_ray_args>(rays));
}

int computeRays(mwhip_exec *exec, uint64_t handle, bool wait)
{
    return computeObject(exec, findRays(exec, handle), "ray query", handle, wait, queueRays);
}

}

// Tail stage: the ONE launch that recomputes every step ray query inside a step
// replay, behind the step views (origins and counts may be a step view's of the
// same replay) and in front of the step gathers (which may read the hits); none
// when no step query is set.
MWHIP_RT int stepRaysStage(mwhip_exec *exec, const LaunchGraph &lg,
                           std::vector<KernelLaunch> &out)
{
    if (lg.isRender || exec->rayKernel == nullptr) return 0;
    mwhip_ray_args args {};
    double bytes = 0;
    const uint32_t items = collectStepBatch(
        exec->extras.stepRays, exec->rays, args, [&](const mwhip_rays_rec &rays) {
            // written: hit_t, hit, normal, status; read: direction, t_max, and
            // per fan world and origin (the trees' bytes depend on the rays)
            bytes += (double)rays.numRays * (28.0 + 16.0) + (double)rays.numFans * 16.0;
        });
    if (args.num_plans == 0) return 0;
    out.push_back(stageLaunch(exec->rayKernel, rayGrid(exec, items), kRayThreads, args, "rays",
                              "rays", bytes));
    return 0;
}

extern "C" int mwhip_set_ray_kernel(mwhip_exec *exec, const void *kernel)
{
    carryStale(exec);
    if (exec == nullptr) return fail(-2, "set_ray_kernel: no executor");
    if (kernel != nullptr) exec->rayKernel = kernel;
    return 0;
}

extern "C" int mwhip_rays_create(mwhip_exec *exec, const mwhip_rays_desc *desc,
                                 uint64_t *rays_out)
{
    carryStale(exec);
    // (every refusal comes before anything is allocated)
    if (exec == nullptr || !exec->stateBuilt || rays_out == nullptr) {
        return fail(-2, "rays_create: no executor state");
    }
    if (desc == nullptr) return fail(-2, "rays_create: no descriptor");
    if (exec->rayKernel == nullptr) {
        return fail(-2, "rays_create: this simulator registered no ray kernel (it sets up no "
                    "broadphase: PhysicsSystem::setupBroadphaseTasks)");
    }
    if (desc->num_fans == 0u || desc->rays_per_fan == 0u) {
        return fail(-2, "rays_create: %u fans of %u rays", desc->num_fans, desc->rays_per_fan);
    }
    if ((uint64_t)desc->num_fans * desc->rays_per_fan > 0x7FFFFFFFull) {
        return fail(-2, "rays_create: %u fans x %u rays is more than %u rays", desc->num_fans,
                    desc->rays_per_fan, 0x7FFFFFFFu);
    }
    const bool by_rule = desc->fans_per_world != 0u;
    const bool own_world = !by_rule && desc->world.src == nullptr;
    const bool own_origin = desc->origin.src == nullptr;
    const int rc = checkGroupSources("rays_create", by_rule, "fans_per_world", desc->world,
                                     desc->count, "origin", desc->origin);
    if (rc != 0) return rc;

    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    std::unique_ptr<mwhip_rays_rec> rays(new mwhip_rays_rec());
    const uint32_t F = desc->num_fans, R = desc->rays_per_fan, N = F * R;
    rays->numFans = F;
    rays->raysPerFan = R;
    rays->numRays = N;
    // (from 8 rays on traceRayShared shares a fan's leaf tests)
    const uint32_t groups_per_fan = R >= 8u ? (R + 31u) / 32u : 0u;
    const uint64_t groups = groups_per_fan != 0u ? (uint64_t)F * groups_per_fan :
                                                   ((uint64_t)N + 31ull) / 32ull;
    rays->items = (uint32_t)((groups + 1ull) / 2ull);

    rays->bytes[MWHIP_RAYS_BUF_WORLD] = own_world ? (uint64_t)F * 4ull : 0ull;
    rays->bytes[MWHIP_RAYS_BUF_ORIGIN] = own_origin ? (uint64_t)F * 12ull : 0ull;
    rays->bytes[MWHIP_RAYS_BUF_DIR] = (uint64_t)N * 12ull;
    rays->bytes[MWHIP_RAYS_BUF_T_MAX] = (uint64_t)N * 4ull;
    rays->bytes[MWHIP_RAYS_BUF_HIT_T] = (uint64_t)N * 4ull;
    rays->bytes[MWHIP_RAYS_BUF_HIT] = (uint64_t)N * 8ull;
    rays->bytes[MWHIP_RAYS_BUF_NORMAL] = (uint64_t)N * 12ull;
    rays->bytes[MWHIP_RAYS_BUF_STATUS] = (uint64_t)N * 4ull;
    uint64_t total = 0;
    bool ok = allocQueryBuffers(*rays, &total);
    if (ok) {
        // t_max starts at +inf; the outputs as a compute leaves a query that
        // met nothing
        ok = hipMemsetD32((hipDeviceptr_t)rays->bufs[MWHIP_RAYS_BUF_T_MAX], 0x7F800000,
                          (size_t)N) == hipSuccess &&
            hipMemset(rays->bufs[MWHIP_RAYS_BUF_HIT], 0xFF, (uint64_t)N * 8ull) == hipSuccess;
    }
    if (ok) {
        mwhip_ray_plan plan {};
        plan.state = exec->stateDev;
        if (!by_rule) {
            resolveItemSource(own_world, rays->bufs[MWHIP_RAYS_BUF_WORLD], 4u, desc->world,
                              &plan.world_src, &plan.world_stride);
        }
        resolveItemSource(false, nullptr, 0u, desc->count, &plan.count_src, &plan.count_stride);
        resolveItemSource(own_origin, rays->bufs[MWHIP_RAYS_BUF_ORIGIN], 12u, desc->origin,
                          &plan.origin_src, &plan.origin_stride);
        plan.dir = (const float *)rays->bufs[MWHIP_RAYS_BUF_DIR];
        plan.t_max = (const float *)rays->bufs[MWHIP_RAYS_BUF_T_MAX];
        plan.hit_t = (float *)rays->bufs[MWHIP_RAYS_BUF_HIT_T];
        plan.hit = (uint32_t *)rays->bufs[MWHIP_RAYS_BUF_HIT];
        plan.normal = (float *)rays->bufs[MWHIP_RAYS_BUF_NORMAL];
        plan.status = (int32_t *)rays->bufs[MWHIP_RAYS_BUF_STATUS];
        plan.num_fans = F;
        plan.rays_per_fan = R;
        plan.fans_per_world = desc->fans_per_world;
        plan.groups_per_fan = groups_per_fan;
        ok = hipMemcpy(rays->planDev, &plan, sizeof(plan), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        return CREATE_FAILED(rays, "rays_create: no device memory for the plan and %llu bytes "
                             "(%u fans of %u rays)", (unsigned long long)total, F, R);
    }
    *rays_out = exec->rays.insert(std::move(rays));
    return 0;
}

extern "C" int mwhip_set_step_rays(mwhip_exec *exec, uint64_t rays, int on)
{
    carryStale(exec);
    if (findRays(exec, rays) == nullptr) return unknownObject("ray query", rays);
    return toggleStepSet(exec, &ReplayExtras::stepRays, rays, on, MWHIP_MAX_STEP_RAYS,
                         "set_step_rays", "step ray queries");
}

extern "C" void mwhip_rays_destroy(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    destroyStepObject(exec, &mwhip_exec::rays, handle, &mwhip_set_step_rays);
}

extern "C" int mwhip_rays_compute(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeRays(exec, handle, true);
}

extern "C" int mwhip_rays_compute_async(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeRays(exec, handle, false);
}

extern "C" void *mwhip_rays_buffer(mwhip_exec *exec, uint64_t handle, uint32_t which,
                                   uint64_t *bytes_out)
{
    return queryBuffer(findRays(exec, handle), "ray query", handle, "rays_buffer",
                       "fans_per_world", which, bytes_out);
}
