// libmadrona_hip.so -- shape queries: S = F x G posed collision shapes, F bundles
// of G shapes that share a world, each tested against the rigid bodies of its
// world with the step's narrowphase; per shape the bodies it would touch and the
// manifold of each (mwhip_shapes_*, include/mwhip.h; DESIGN.md §39;
// madrona_amd/shape_ref.py is the definition).
//
// This file is the host side only, a sibling of contact_query.hip.  The kernel,
// shapeQueryKernel, is compiled into the simulator's code object
// (include/madrona/phys_impl/shape_query.inl), where the narrowphase lives;
// PhysicsSystem::setupPhysicsStepTasks registers its host stub
// (mwhip_set_shape_kernel) and the runtime launches it.  What the two code
// objects share is the POD pair mwhip_shape_plan / mwhip_shape_args of mwhip.h.
// A query owns a device-resident plan and ONE allocation with its owned inputs
// (world and exclude unless a source was given; object, position, rotation and
// scale always) and its outputs, 256-byte aligned each.  Sources are read on the
// device when the kernel runs, as a ray query's.  The executor owns one scratch
// block for the generic single-lane routine, a slot per wavefront of the
// largest grid, made by the first create and shared by every shape query:
// two wavefronts of a launch may be in the same world, so the world's slot of
// the step's scratch will not do, and computes are stream-ordered.
#include "tree_query.hpp"

namespace {

constexpr uint32_t kShapeThreads = 256;
constexpr uint32_t kShapeWaves = kShapeThreads / 64u;
// Registers hold this kernel to one workgroup per CU at a time,
// yet the grid is capped at 8 workgroups per CU, the contact kernel's cap, not
// at 1: a bundle's work depends on what its shapes meet, and with eight times
// as many workgroups as can be resident the dispatcher hands the next one to
// whichever CU finishes first, where a grid of resident workgroups would have
// each stride over a fixed eighth of the bundles.  The times of
// profiles/shape_query_times.md are taken at this cap.  The price is the
// scratch block: a slot per wavefront of that grid, 8 x 4 x numCUs slots of
// 3.5 KiB (28 MiB at 256 CUs), eight times what is resident at once.
constexpr uint32_t kShapeBlocksPerCU = 8;

}

struct mwhip_shapes_rec : TreeQueryRec<mwhip_shape_plan, MWHIP_SHAPES_NUM_BUFS> {
    uint32_t numBundles = 0;
    uint32_t numShapes = 0;
    uint32_t maxHits = 0;
};

namespace {

mwhip_shapes_rec *findShapes(mwhip_exec *exec, uint64_t handle)
{
    return findObject(exec != nullptr ? &exec->shapes : nullptr, handle);
}

// (a work item is a BUNDLE; wavefronts stride over the bundles of all plans)
dim3 shapeGrid(mwhip_exec *exec, uint32_t bundles)
{
    return waveGrid(exec, bundles, kShapeWaves, kShapeBlocksPerCU);
}

// the wavefronts of the largest grid shapeGrid can return
uint32_t shapeScratchWaves(const mwhip_exec *exec)
{
    return std::max(exec->numCUs, 1u) * kShapeBlocksPerCU * kShapeWaves;
}

int queueShapes(mwhip_exec *exec, mwhip_shapes_rec &shapes)
{
    return queueBatch(exec, exec->shapeKernel, shapeGrid(exec, shapes.items), kShapeThreads,
                      singleBatch<mwhip_shape_args>(shapes));
}

int computeShapes(mwhip_exec *exec, uint64_t handle, bool wait)
{
    return computeObject(exec, findShapes(exec, handle), "shape query", handle, wait,
                         queueShapes);
}

}

// Tail stage: the ONE launch that recomputes every step shape query inside a
// step replay, directly behind the step contact queries and in front of the
// step gathers (which may read the hits); none when no step query is set.  It
// reads the tables and writes only the queries' own buffers and the executor's
// shape scratch, so it has no say in whether a steady replay drops its carried
// launches.
MWHIP_RT int stepShapesStage(mwhip_exec *exec, const LaunchGraph &lg,
                             std::vector<KernelLaunch> &out)
{
    if (lg.isRender || exec->shapeKernel == nullptr) return 0;
    mwhip_shape_args args {};
    double bytes = 0;
    const uint32_t items = collectStepBatch(
        exec->extras.stepShapes, exec->shapes, args, [&](const mwhip_shapes_rec &shapes) {
            // written: status, count and every hit slot (8 + 4 + 4 + 12 + 64
            // bytes); read: object, pose, exclude and per bundle the world.  The
            // bodies' bytes depend on what the shapes meet and are not counted.
            bytes += (double)shapes.numShapes * (8.0 + 92.0 * (double)shapes.maxHits + 52.0) +
                (double)shapes.numBundles * 4.0;
        });
    if (args.num_plans == 0) return 0;
    out.push_back(stageLaunch(exec->shapeKernel, shapeGrid(exec, items), kShapeThreads, args,
                              "shapes", "shapes", bytes));
    return 0;
}

extern "C" int mwhip_set_shape_kernel(mwhip_exec *exec, const void *kernel,
                                      uint32_t scratch_bytes_per_wavefront)
{
    carryStale(exec);
    if (exec == nullptr) return fail(-2, "set_shape_kernel: no executor");
    // (a wavefront without a scratch slot serves nothing, and a compute must
    // rewrite every output)
    if (kernel != nullptr && scratch_bytes_per_wavefront == 0u) {
        return fail(-2, "set_shape_kernel: scratch_bytes_per_wavefront is 0");
    }
    // (the stride stays what the first registration said once the block exists)
    if (kernel != nullptr && exec->shapeScratch == nullptr) {
        exec->shapeKernel = kernel;
        exec->shapeScratchBytes = (scratch_bytes_per_wavefront + 255u) & ~255u;
    } else if (kernel != nullptr) {
        exec->shapeKernel = kernel;
    }
    return 0;
}

extern "C" int mwhip_shapes_create(mwhip_exec *exec, const mwhip_shapes_desc *desc,
                                   uint64_t *shapes_out)
{
    carryStale(exec);
    // (every refusal comes before anything is allocated)
    if (exec == nullptr || !exec->stateBuilt || shapes_out == nullptr) {
        return fail(-2, "shapes_create: no executor state");
    }
    if (desc == nullptr) return fail(-2, "shapes_create: no descriptor");
    if (exec->shapeKernel == nullptr) {
        return fail(-2, "shapes_create: this simulator registered no shape kernel (it sets up no "
                    "rigid-body step: PhysicsSystem::setupPhysicsStepTasks)");
    }
    if (desc->num_bundles == 0u || desc->shapes_per_bundle == 0u || desc->max_hits == 0u ||
            desc->num_objects == 0u) {
        return fail(-2, "shapes_create: %u bundles of %u shapes with %u hits each, %u objects",
                    desc->num_bundles, desc->shapes_per_bundle, desc->max_hits,
                    desc->num_objects);
    }
    const uint64_t num_shapes = (uint64_t)desc->num_bundles * desc->shapes_per_bundle;
    if (num_shapes > 0x7FFFFFFFull || num_shapes * desc->max_hits > 0x7FFFFFFFull) {
        return fail(-2, "shapes_create: %u bundles x %u shapes x %u hits is more than %u handles",
                    desc->num_bundles, desc->shapes_per_bundle, desc->max_hits, 0x7FFFFFFFu);
    }
    if ((desc->flags & ~MWHIP_SHAPES_PLAIN) != 0u) {
        return fail(-2, "shapes_create: unknown flags 0x%x", desc->flags);
    }
    const bool by_rule = desc->bundles_per_world != 0u;
    const bool own_world = !by_rule && desc->world.src == nullptr;
    const bool own_exclude = desc->exclude.src == nullptr;
    int rc = 0;
    if (!by_rule && desc->world.src != nullptr) {
        rc = checkItemSource("shapes_create", "world", desc->world, 4u);
    }
    if (rc == 0 && desc->count.src != nullptr) {
        if (!by_rule) {
            return fail(-2, "shapes_create: a count source needs bundles_per_world > 0");
        }
        rc = checkItemSource("shapes_create", "count", desc->count, 4u);
    }
    if (rc == 0 && desc->exclude.src != nullptr) {
        rc = checkItemSource("shapes_create", "exclude", desc->exclude, 8u);
    }
    if (rc != 0) return rc;

    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    // the executor's scratch block, once
    if (exec->shapeScratch == nullptr && exec->shapeScratchBytes != 0u) {
        const uint32_t waves = shapeScratchWaves(exec);
        void *block = nullptr;
        if (hipMalloc(&block, (size_t)waves * exec->shapeScratchBytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(-10, "shapes_create: no device memory for %u x %u bytes of scratch",
                        waves, exec->shapeScratchBytes);
        }
        exec->shapeScratch = (char *)block;
        exec->shapeScratchWaves = waves;
        exec->allocations.push_back(block);
    }

    std::unique_ptr<mwhip_shapes_rec> shapes(new mwhip_shapes_rec());
    const uint32_t F = desc->num_bundles, G = desc->shapes_per_bundle, K = desc->max_hits;
    const uint32_t S = (uint32_t)num_shapes;
    shapes->numBundles = F;
    shapes->numShapes = S;
    shapes->maxHits = K;
    shapes->items = F;

    const uint64_t slots = (uint64_t)S * K;
    shapes->bytes[MWHIP_SHAPES_BUF_WORLD] = own_world ? (uint64_t)F * 4ull : 0ull;
    shapes->bytes[MWHIP_SHAPES_BUF_EXCLUDE] = own_exclude ? (uint64_t)S * 8ull : 0ull;
    shapes->bytes[MWHIP_SHAPES_BUF_OBJECT] = (uint64_t)S * 4ull;
    shapes->bytes[MWHIP_SHAPES_BUF_POSITION] = (uint64_t)S * 12ull;
    shapes->bytes[MWHIP_SHAPES_BUF_ROTATION] = (uint64_t)S * 16ull;
    shapes->bytes[MWHIP_SHAPES_BUF_SCALE] = (uint64_t)S * 12ull;
    shapes->bytes[MWHIP_SHAPES_BUF_STATUS] = (uint64_t)S * 4ull;
    shapes->bytes[MWHIP_SHAPES_BUF_COUNT] = (uint64_t)S * 4ull;
    shapes->bytes[MWHIP_SHAPES_BUF_HITS] = slots * 8ull;
    shapes->bytes[MWHIP_SHAPES_BUF_SHAPE_IS_REF] = slots * 4ull;
    shapes->bytes[MWHIP_SHAPES_BUF_NUM_POINTS] = slots * 4ull;
    shapes->bytes[MWHIP_SHAPES_BUF_NORMAL] = slots * 12ull;
    shapes->bytes[MWHIP_SHAPES_BUF_POINTS] = slots * 64ull;
    uint64_t total = 0;
    bool ok = allocQueryBuffers(*shapes, &total);
    if (ok) {
        // the outputs as a compute leaves a query whose shapes met nothing
        ok = hipMemset(shapes->bufs[MWHIP_SHAPES_BUF_HITS], 0xFF,
                       shapes->bytes[MWHIP_SHAPES_BUF_HITS]) == hipSuccess;
    }
    if (ok && own_exclude) {
        // Entity::none()
        ok = hipMemset(shapes->bufs[MWHIP_SHAPES_BUF_EXCLUDE], 0xFF,
                       shapes->bytes[MWHIP_SHAPES_BUF_EXCLUDE]) == hipSuccess;
    }
    if (ok) {
        // the identity pose at unit scale
        std::vector<float> rotation((size_t)S * 4u, 0.f);
        for (uint32_t s = 0; s < S; s++) rotation[(size_t)s * 4u] = 1.f;
        const std::vector<float> scale((size_t)S * 3u, 1.f);
        ok = hipMemcpy(shapes->bufs[MWHIP_SHAPES_BUF_ROTATION], rotation.data(),
                       rotation.size() * 4u, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(shapes->bufs[MWHIP_SHAPES_BUF_SCALE], scale.data(), scale.size() * 4u,
                      hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) {
        mwhip_shape_plan plan {};
        plan.state = exec->stateDev;
        if (!by_rule) {
            resolveItemSource(own_world, shapes->bufs[MWHIP_SHAPES_BUF_WORLD], 4u, desc->world,
                              &plan.world_src, &plan.world_stride);
        }
        resolveItemSource(false, nullptr, 0u, desc->count, &plan.count_src, &plan.count_stride);
        resolveItemSource(own_exclude, shapes->bufs[MWHIP_SHAPES_BUF_EXCLUDE], 8u, desc->exclude,
                          &plan.exclude_src, &plan.exclude_stride);
        plan.object = (const int32_t *)shapes->bufs[MWHIP_SHAPES_BUF_OBJECT];
        plan.position = (const float *)shapes->bufs[MWHIP_SHAPES_BUF_POSITION];
        plan.rotation = (const float *)shapes->bufs[MWHIP_SHAPES_BUF_ROTATION];
        plan.scale = (const float *)shapes->bufs[MWHIP_SHAPES_BUF_SCALE];
        plan.status = (int32_t *)shapes->bufs[MWHIP_SHAPES_BUF_STATUS];
        plan.count = (int32_t *)shapes->bufs[MWHIP_SHAPES_BUF_COUNT];
        plan.hits = (uint32_t *)shapes->bufs[MWHIP_SHAPES_BUF_HITS];
        plan.shape_is_ref = (int32_t *)shapes->bufs[MWHIP_SHAPES_BUF_SHAPE_IS_REF];
        plan.num_points = (int32_t *)shapes->bufs[MWHIP_SHAPES_BUF_NUM_POINTS];
        plan.normal = (float *)shapes->bufs[MWHIP_SHAPES_BUF_NORMAL];
        plan.points = (float *)shapes->bufs[MWHIP_SHAPES_BUF_POINTS];
        plan.scratch = exec->shapeScratch;
        plan.num_bundles = F;
        plan.shapes_per_bundle = G;
        plan.max_hits = K;
        plan.num_objects = desc->num_objects;
        plan.bundles_per_world = desc->bundles_per_world;
        plan.flags = desc->flags;
        plan.scratch_stride = exec->shapeScratchBytes;
        plan.scratch_waves = exec->shapeScratchWaves;
        ok = hipMemcpy(shapes->planDev, &plan, sizeof(plan), hipMemcpyHostToDevice) ==
            hipSuccess;
    }
    if (!ok) {
        return CREATE_FAILED(shapes, "shapes_create: no device memory for the plan and %llu bytes "
                             "(%u bundles of %u shapes, %u hits each)", (unsigned long long)total,
                             F, G, K);
    }
    *shapes_out = exec->shapes.insert(std::move(shapes));
    return 0;
}

extern "C" int mwhip_set_step_shapes(mwhip_exec *exec, uint64_t shapes, int on)
{
    carryStale(exec);
    if (findShapes(exec, shapes) == nullptr) return unknownObject("shape query", shapes);
    return toggleStepSet(exec, &ReplayExtras::stepShapes, shapes, on, MWHIP_MAX_STEP_SHAPES,
                         "set_step_shapes", "step shape queries");
}

extern "C" void mwhip_shapes_destroy(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    destroyStepObject(exec, &mwhip_exec::shapes, handle, &mwhip_set_step_shapes);
}

extern "C" int mwhip_shapes_compute(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeShapes(exec, handle, true);
}

extern "C" int mwhip_shapes_compute_async(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeShapes(exec, handle, false);
}

extern "C" void *mwhip_shapes_buffer(mwhip_exec *exec, uint64_t handle, uint32_t which,
                                     uint64_t *bytes_out)
{
    return queryBuffer(findShapes(exec, handle), "shape query", handle, "shapes_buffer",
                       "bundles_per_world", which, bytes_out);
}
