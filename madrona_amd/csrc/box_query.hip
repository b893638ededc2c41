// libmadrona_hip.so -- box queries: B = F x G boxes, F bundles of G boxes that
// share a world and a centre, tested through the worlds' broadphase BVHs; per
// box the whole list of the entities PhysicsSystem::findEntitiesWithinAABB
// reports (mwhip_boxes_*, include/mwhip.h; madrona_amd/box_ref.py
// is the definition).
//
// This file is the host side only, a sibling of ray_query.hip.  The kernel,
// boxQueryKernel, is compiled into the simulator's code object
// (include/madrona/phys_impl/box_query.inl), where findEntitiesWithinAABB and
// the hull test live; PhysicsSystem::setupBroadphaseTasks registers its host
// stub (mwhip_set_box_kernel) and the runtime launches it.  What the two code
// objects share is the POD pair mwhip_box_plan / mwhip_box_args of mwhip.h.
// A query owns a device-resident plan and ONE allocation with its owned inputs
// (world and centre unless a source was given; lo and hi always) and its outputs
// (status, count, hits), 256-byte aligned each.  Sources are read on the device
// when the kernel runs, as a ray query's.  What the two share is in
// tree_query.hpp.
#include "tree_query.hpp"

namespace {

constexpr uint32_t kBoxThreads = 256;
constexpr uint32_t kBoxWaves = kBoxThreads / 64u;

}

struct mwhip_boxes_rec : TreeQueryRec<mwhip_box_plan, MWHIP_BOXES_NUM_BUFS> {
    uint32_t numBundles = 0;
    uint32_t numBoxes = 0;
    uint32_t maxHits = 0;
};

namespace {

mwhip_boxes_rec *findBoxes(mwhip_exec *exec, uint64_t handle)
{
    return findObject(exec != nullptr ? &exec->boxes : nullptr, handle);
}

// (wavefronts stride over the items; the cap of 8 workgroups per CU is the ray
// kernel's -- registers hold this kernel to 3 wavefronts per SIMD, three
// workgroups per CU at a time: DESIGN.md §35)
dim3 boxGrid(mwhip_exec *exec, uint32_t items)
{
    return waveGrid(exec, items, kBoxWaves, 8u);
}

int queueBoxes(mwhip_exec *exec, mwhip_boxes_rec &boxes)
{
    return queueBatch(exec, exec->boxKernel, boxGrid(exec, boxes.items), kBoxThreads,
                      singleBatch<mwhip_box_args>(boxes));
}

int computeBoxes(mwhip_exec *exec, uint64_t handle, bool wait)
{
    return computeObject(exec, findBoxes(exec, handle), "box query", handle, wait, queueBoxes);
}

}

// Tail stage: the ONE launch that recomputes every step box query inside a step
// replay, directly behind the step ray queries (hence behind the step views:
// centres and counts may be a step view's of the same replay) and in front of
// the step gathers (which may read the hits); none when no step query is set.
// It reads the trees and the tables and writes only the queries' own buffers, so
// it has no say in whether a steady replay drops its carried launches.
MWHIP_RT int stepBoxesStage(mwhip_exec *exec, const LaunchGraph &lg,
                            std::vector<KernelLaunch> &out)
{
    if (lg.isRender || exec->boxKernel == nullptr) return 0;
    mwhip_box_args args {};
    double bytes = 0;
    const uint32_t items = collectStepBatch(
        exec->extras.stepBoxes, exec->boxes, args, [&](const mwhip_boxes_rec &boxes) {
            // written: status, count and every hit slot; read: lo, hi, and per
            // bundle world and centre (the trees' and the bodies' bytes depend
            // on the boxes and are not counted)
            bytes += (double)boxes.numBoxes * (8.0 + 8.0 * (double)boxes.maxHits + 24.0) +
                (double)boxes.numBundles * 16.0;
        });
    if (args.num_plans == 0) return 0;
    out.push_back(stageLaunch(exec->boxKernel, boxGrid(exec, items), kBoxThreads, args, "boxes",
                              "boxes", bytes));
    return 0;
}

extern "C" int mwhip_set_box_kernel(mwhip_exec *exec, const void *kernel)
{
    carryStale(exec);
    if (exec == nullptr) return fail(-2, "set_box_kernel: no executor");
    if (kernel != nullptr) exec->boxKernel = kernel;
    return 0;
}

extern "C" int mwhip_boxes_create(mwhip_exec *exec, const mwhip_boxes_desc *desc,
                                  uint64_t *boxes_out)
{
    carryStale(exec);
    // (every refusal comes before anything is allocated)
    if (exec == nullptr || !exec->stateBuilt || boxes_out == nullptr) {
        return fail(-2, "boxes_create: no executor state");
    }
    if (desc == nullptr) return fail(-2, "boxes_create: no descriptor");
    if (exec->boxKernel == nullptr) {
        return fail(-2, "boxes_create: this simulator registered no box kernel (it sets up no "
                    "broadphase: PhysicsSystem::setupBroadphaseTasks)");
    }
    if (desc->num_bundles == 0u || desc->boxes_per_bundle == 0u || desc->max_hits == 0u) {
        return fail(-2, "boxes_create: %u bundles of %u boxes with %u hits each",
                    desc->num_bundles, desc->boxes_per_bundle, desc->max_hits);
    }
    const uint64_t num_boxes = (uint64_t)desc->num_bundles * desc->boxes_per_bundle;
    if (num_boxes > 0x7FFFFFFFull || num_boxes * desc->max_hits > 0x7FFFFFFFull) {
        return fail(-2, "boxes_create: %u bundles x %u boxes x %u hits is more than %u handles",
                    desc->num_bundles, desc->boxes_per_bundle, desc->max_hits, 0x7FFFFFFFu);
    }
    if ((desc->flags & ~MWHIP_BOXES_PACKED) != 0u) {
        return fail(-2, "boxes_create: unknown flags 0x%x", desc->flags);
    }
    const bool by_rule = desc->bundles_per_world != 0u;
    const bool own_world = !by_rule && desc->world.src == nullptr;
    const bool own_centre = desc->centre.src == nullptr;
    const int rc = checkGroupSources("boxes_create", by_rule, "bundles_per_world", desc->world,
                                     desc->count, "centre", desc->centre);
    if (rc != 0) return rc;

    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    std::unique_ptr<mwhip_boxes_rec> boxes(new mwhip_boxes_rec());
    const uint32_t F = desc->num_bundles, G = desc->boxes_per_bundle, K = desc->max_hits;
    const uint32_t B = (uint32_t)num_boxes;
    boxes->numBundles = F;
    boxes->numBoxes = B;
    boxes->maxHits = K;
    const bool packed = (desc->flags & MWHIP_BOXES_PACKED) != 0u;
    // cooperative: a group of 32 lanes per chunk of up to 32 boxes of a bundle,
    // two groups per wavefront; packed: 64 boxes per wavefront
    const uint32_t chunks = packed ? 0u : (G + 31u) / 32u;
    const uint64_t groups = (uint64_t)F * chunks;
    boxes->items = packed ? (B + 63u) / 64u : (uint32_t)((groups + 1ull) / 2ull);

    boxes->bytes[MWHIP_BOXES_BUF_WORLD] = own_world ? (uint64_t)F * 4ull : 0ull;
    boxes->bytes[MWHIP_BOXES_BUF_CENTRE] = own_centre ? (uint64_t)F * 12ull : 0ull;
    boxes->bytes[MWHIP_BOXES_BUF_LO] = (uint64_t)B * 12ull;
    boxes->bytes[MWHIP_BOXES_BUF_HI] = (uint64_t)B * 12ull;
    boxes->bytes[MWHIP_BOXES_BUF_STATUS] = (uint64_t)B * 4ull;
    boxes->bytes[MWHIP_BOXES_BUF_COUNT] = (uint64_t)B * 4ull;
    boxes->bytes[MWHIP_BOXES_BUF_HITS] = (uint64_t)B * K * 8ull;
    uint64_t total = 0;
    bool ok = allocQueryBuffers(*boxes, &total);
    if (ok) {
        // the outputs as a compute leaves a query whose boxes met nothing
        ok = hipMemset(boxes->bufs[MWHIP_BOXES_BUF_HITS], 0xFF,
                       boxes->bytes[MWHIP_BOXES_BUF_HITS]) == hipSuccess;
    }
    if (ok) {
        mwhip_box_plan plan {};
        plan.state = exec->stateDev;
        if (!by_rule) {
            resolveItemSource(own_world, boxes->bufs[MWHIP_BOXES_BUF_WORLD], 4u, desc->world,
                              &plan.world_src, &plan.world_stride);
        }
        resolveItemSource(false, nullptr, 0u, desc->count, &plan.count_src, &plan.count_stride);
        resolveItemSource(own_centre, boxes->bufs[MWHIP_BOXES_BUF_CENTRE], 12u, desc->centre,
                          &plan.centre_src, &plan.centre_stride);
        plan.lo = (const float *)boxes->bufs[MWHIP_BOXES_BUF_LO];
        plan.hi = (const float *)boxes->bufs[MWHIP_BOXES_BUF_HI];
        plan.status = (int32_t *)boxes->bufs[MWHIP_BOXES_BUF_STATUS];
        plan.count = (int32_t *)boxes->bufs[MWHIP_BOXES_BUF_COUNT];
        plan.hits = (uint32_t *)boxes->bufs[MWHIP_BOXES_BUF_HITS];
        plan.num_bundles = F;
        plan.boxes_per_bundle = G;
        plan.max_hits = K;
        plan.bundles_per_world = desc->bundles_per_world;
        plan.chunks_per_bundle = chunks;
        ok = hipMemcpy(boxes->planDev, &plan, sizeof(plan), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        return CREATE_FAILED(boxes, "boxes_create: no device memory for the plan and %llu bytes "
                             "(%u bundles of %u boxes, %u hits each)", (unsigned long long)total,
                             F, G, K);
    }
    *boxes_out = exec->boxes.insert(std::move(boxes));
    return 0;
}

extern "C" int mwhip_set_step_boxes(mwhip_exec *exec, uint64_t boxes, int on)
{
    carryStale(exec);
    if (findBoxes(exec, boxes) == nullptr) return unknownObject("box query", boxes);
    return toggleStepSet(exec, &ReplayExtras::stepBoxes, boxes, on, MWHIP_MAX_STEP_BOXES,
                         "set_step_boxes", "step box queries");
}

extern "C" void mwhip_boxes_destroy(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    destroyStepObject(exec, &mwhip_exec::boxes, handle, &mwhip_set_step_boxes);
}

extern "C" int mwhip_boxes_compute(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeBoxes(exec, handle, true);
}

extern "C" int mwhip_boxes_compute_async(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeBoxes(exec, handle, false);
}

extern "C" void *mwhip_boxes_buffer(mwhip_exec *exec, uint64_t handle, uint32_t which,
                                    uint64_t *bytes_out)
{
    return queryBuffer(findBoxes(exec, handle), "box query", handle, "boxes_buffer",
                       "bundles_per_world", which, bytes_out);
}
