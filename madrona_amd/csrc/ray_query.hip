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
// read on the device when the kernel runs, as a gather's.
#include "exec_internal.hpp"

namespace {

constexpr uint32_t kRayThreads = 256;
constexpr uint32_t kRayWaves = kRayThreads / 64u;

}

struct mwhip_rays_rec {
    uint64_t handle = 0;
    uint32_t numFans = 0;
    uint32_t raysPerFan = 0;
    uint32_t numRays = 0;
    uint32_t items = 0;         // wavefront work items
    char *bufs[MWHIP_RAYS_NUM_BUFS] = {};       // into bufDev; null: not owned
    uint64_t bytes[MWHIP_RAYS_NUM_BUFS] = {};
    mwhip_ray_plan *planDev = nullptr;
    char *bufDev = nullptr;

    ~mwhip_rays_rec()
    {
        if (planDev != nullptr) (void)hipFree(planDev);
        if (bufDev != nullptr) (void)hipFree(bufDev);
    }
};

namespace {

mwhip_rays_rec *findRays(mwhip_exec *exec, uint64_t handle)
{
    return findObject(exec != nullptr ? &exec->rays : nullptr, handle);
}

// (four workgroups of 39 KB of LDS fit a CU; wavefronts stride over the items)
dim3 rayGrid(mwhip_exec *exec, uint32_t items)
{
    const uint32_t blocks = (items + kRayWaves - 1u) / kRayWaves;
    return dim3(std::max(std::min(blocks, std::max(exec->numCUs, 1u) * 8u), 1u), 1, 1);
}

int queueRays(mwhip_exec *exec, mwhip_rays_rec &rays)
{
    mwhip_ray_args args {};
    args.num_plans = 1;
    args.items[0] = rays.items;
    args.plans[0] = rays.planDev;
    void *argv[] = { &args };
    HIPCHK(hipLaunchKernel(exec->rayKernel, rayGrid(exec, rays.items), dim3(kRayThreads), argv,
                           0, exec->stream));
    return 0;
}

int computeRays(mwhip_exec *exec, uint64_t handle, bool wait)
{
    mwhip_rays_rec *rays = findRays(exec, handle);
    if (rays == nullptr) return unknownObject("ray query", handle);
    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    return finishQueued(exec, queueRays(exec, *rays), wait);
}

int checkRaySource(const char *name, const mwhip_ray_source &source, uint32_t item_bytes)
{
    return checkItemSource("rays_create", name, source, item_bytes);
}

}

// what a create refuses about a source of `item_bytes` per record (box queries
// take the same sources: box_query.hip)
MWHIP_RT int checkItemSource(const char *who, const char *name, const mwhip_ray_source &source,
                             uint32_t item_bytes)
{
    if (((uint64_t)source.src & 3ull) != 0ull || source.record_bytes % 4u != 0u ||
            source.first_byte % 4u != 0u) {
        return fail(-2, "%s: %s: src %p, record_bytes %u and first_byte %u must be "
                    "multiples of 4", who, name, source.src, source.record_bytes,
                    source.first_byte);
    }
    if ((uint64_t)source.first_byte + item_bytes > (uint64_t)source.record_bytes) {
        return fail(-2, "%s: %s: %u bytes from byte %u do not fit a record of %u bytes", who,
                    name, item_bytes, source.first_byte, source.record_bytes);
    }
    return 0;
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
    uint32_t items = 0;
    double bytes = 0;
    for (uint64_t handle : exec->extras.stepRays) {
        mwhip_rays_rec *rays = findRays(exec, handle);
        if (rays == nullptr || args.num_plans >= MWHIP_MAX_STEP_RAYS) continue;
        args.items[args.num_plans] = rays->items;
        args.plans[args.num_plans] = rays->planDev;
        args.num_plans += 1;
        items += rays->items;
        // written: hit_t, hit, normal, status; read: direction, t_max, and per
        // fan world and origin (the trees' bytes depend on the rays)
        bytes += (double)rays->numRays * (28.0 + 16.0) + (double)rays->numFans * 16.0;
    }
    if (args.num_plans == 0) return 0;

    KernelLaunch k;
    static_assert(sizeof(mwhip_ray_args) <= sizeof(k.argStorage));
    k.fn = exec->rayKernel;
    k.grid = rayGrid(exec, items);
    k.block = dim3(kRayThreads, 1, 1);
    k.setArgs(args);
    k.name = "rays";
    k.role = "rays";
    k.kind = MWHIP_NODE_RECYCLE;
    k.fixedBytes = bytes;
    out.push_back(k);
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
    int rc = 0;
    if (!by_rule && !own_world) rc = checkRaySource("world", desc->world, 4u);
    if (rc == 0 && desc->count.src != nullptr) {
        if (!by_rule) {
            return fail(-2, "rays_create: a count source needs fans_per_world > 0");
        }
        rc = checkRaySource("count", desc->count, 4u);
    }
    if (rc == 0 && !own_origin) rc = checkRaySource("origin", desc->origin, 12u);
    if (rc != 0) return rc;

    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    std::unique_ptr<mwhip_rays_rec> rays(new mwhip_rays_rec {});
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
    uint64_t offsets[MWHIP_RAYS_NUM_BUFS];
    uint64_t total = 0;
    for (uint32_t b = 0; b < MWHIP_RAYS_NUM_BUFS; b++) {
        offsets[b] = total;
        total += (rays->bytes[b] + 255ull) & ~255ull;
    }

    bool ok = hipMalloc((void **)&rays->bufDev, total) == hipSuccess &&
        hipMalloc((void **)&rays->planDev, sizeof(mwhip_ray_plan)) == hipSuccess &&
        hipMemset(rays->bufDev, 0, total) == hipSuccess;
    if (ok) {
        for (uint32_t b = 0; b < MWHIP_RAYS_NUM_BUFS; b++) {
            if (rays->bytes[b] != 0ull) rays->bufs[b] = rays->bufDev + offsets[b];
        }
        // t_max starts at +inf; the outputs as a compute leaves a query that
        // met nothing
        ok = hipMemsetD32((hipDeviceptr_t)rays->bufs[MWHIP_RAYS_BUF_T_MAX], 0x7F800000,
                          (size_t)N) == hipSuccess &&
            hipMemset(rays->bufs[MWHIP_RAYS_BUF_HIT], 0xFF, (uint64_t)N * 8ull) == hipSuccess;
    }
    if (ok) {
        mwhip_ray_plan plan {};
        plan.state = exec->stateDev;
        if (own_world) {
            plan.world_src = rays->bufs[MWHIP_RAYS_BUF_WORLD];
            plan.world_stride = 4u;
        } else if (!by_rule) {
            plan.world_src = (const char *)desc->world.src + desc->world.first_byte;
            plan.world_stride = desc->world.record_bytes;
        }
        if (desc->count.src != nullptr) {
            plan.count_src = (const char *)desc->count.src + desc->count.first_byte;
            plan.count_stride = desc->count.record_bytes;
        }
        if (own_origin) {
            plan.origin_src = rays->bufs[MWHIP_RAYS_BUF_ORIGIN];
            plan.origin_stride = 12u;
        } else {
            plan.origin_src = (const char *)desc->origin.src + desc->origin.first_byte;
            plan.origin_stride = desc->origin.record_bytes;
        }
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
    const std::vector<uint64_t> &step_rays = exec->extras.stepRays;
    const bool is_on = std::find(step_rays.begin(), step_rays.end(), rays) != step_rays.end();
    if (is_on == (on != 0)) return 0;
    if (on != 0 && step_rays.size() >= MWHIP_MAX_STEP_RAYS) {
        return fail(-2, "set_step_rays: %u step ray queries are set already (at most %u)",
                    (uint32_t)step_rays.size(), (uint32_t)MWHIP_MAX_STEP_RAYS);
    }
    return changeReplayExtras(exec, [rays, on](ReplayExtras &extras) {
        std::vector<uint64_t> &set = extras.stepRays;
        if (on != 0) {
            set.push_back(rays);
        } else {
            set.erase(std::find(set.begin(), set.end(), rays));
        }
        return 0;
    });
}

extern "C" void mwhip_rays_destroy(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    if (findRays(exec, handle) == nullptr) return;
    (void)hipSetDevice(exec->cfg.gpu_id);
    // (the step graphs must stop naming its buffers before they go; if they
    // could not be rebuilt without it, it stays until mwhip_destroy)
    if (mwhip_set_step_rays(exec, handle, 0) != 0) return;
    (void)hipStreamSynchronize(exec->stream);
    exec->rays.erase(handle);
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
    mwhip_rays_rec *rays = findRays(exec, handle);
    if (rays == nullptr) {
        (void)unknownObject("ray query", handle);
        return nullptr;
    }
    if (which >= MWHIP_RAYS_NUM_BUFS) {
        (void)fail(-2, "rays_buffer: buffer %u of %u", which, (uint32_t)MWHIP_RAYS_NUM_BUFS);
        return nullptr;
    }
    if (rays->bufs[which] == nullptr) {
        (void)fail(-2, "rays_buffer: buffer %u is not owned (a source or fans_per_world was "
                   "given)", which);
        return nullptr;
    }
    if (bytes_out != nullptr) *bytes_out = rays->bytes[which];
    return rays->bufs[which];
}
