// libmadrona_hip.so -- entity gathers: N entity handles read from device memory
// turned into, per listed component, the cell the entity each handle names has,
// plus the archetype and the world that entity lives in (mwhip_gather_*,
// include/mwhip.h; madrona_amd/gather_ref.py is the definition).
//
// A gather owns a device-resident PLAN -- where the handles are (a run of
// records with a run of Entity cells in each), per listed component its id, its
// cell bytes and its buffer -- and one allocation that holds the buffers and the
// two int32 outputs.  Everything about the ECS is read on the device when the
// kernel runs, through the executor's EcsState: entityCapacity, the entity
// slots, the table headers (numRows, columns[0] / columns[1]) and colPtr.  So a
// plan made before a table or the entity store grew, or before a sort swapped a
// column with its twin, is still right.
//   entityGatherKernel   a wavefront owns 64 consecutive handles, a lane one;
//                        wavefronts stride over the (gather, 64 handles) items
//                        of up to MWHIP_MAX_STEP_GATHERS gathers passed by value.
// A lane
//   1. loads its handle as two dwords (the source is 4-byte aligned, no more);
//   2. goes from the handle to a row through the entity store, as
//      Context::get<T>(e) does, but trusts nothing on the way -- the handle is
//      arbitrary bits -- and dereferences nothing behind a check that failed:
//      0 <= id < entityCapacity, slot.gen == gen, archetype < numArchetypeSlots
//      and registered, 0 <= row < numRows, the row's own Entity cell == the
//      handle and its WorldID cell != -1 (gather_ref.py's rule, which is a
//      statement about the TABLES: the slot only says where to look);
//   3. stores archetype and world (-1, -1 for a handle that names nothing);
//   4. per listed component reads its column's base from
//      colPtr[archetype * numComponentSlots + component] (null: the table has
//      no such column) and the wave copies the 64 cells with lane teams: T = the
//      power of two >= ceil(cell bytes / 16), at most 64, lanes per cell,
//      64 / T cells per pass, the owner lane's source pointer fetched with a
//      cross-lane read; cells whose pointer is null are zeroed by the same lanes.
// The 64 slot loads of a wave are independent and in flight together; a wave's
// destination is one contiguous run of 64 cells of a 256-byte aligned buffer.
// No atomics, no LDS, no spin-waits, no workgroup waits for another.
#include "exec_internal.hpp"
#include "entity_resolve.hpp"
#include "world_team.hpp"

namespace {

constexpr uint32_t kGatherThreads = 256;
constexpr uint32_t kGatherWaves = kGatherThreads / 64u;

struct GatherPlanColumn {
    char *dst;              // [numHandles][cellBytes]
    uint32_t component;     // < numComponentSlots (checked by create)
    uint32_t cellBytes;
    uint32_t teamLanes;     // T: a power of two, 1 .. 64
    uint32_t pad_;
};

struct GatherPlan {
    const EcsState *state;  // on the device
    HandleSource source;    // numRecords records of the caller's
    int32_t *archetypes;    // [numHandles]
    int32_t *worlds;        // [numHandles]
    uint32_t numHandles;    // N = numRecords * perRecord <= 2^31 - 1
    uint32_t numColumns;
    GatherPlanColumn columns[MWHIP_GATHER_MAX_COLUMNS];
};

// by value in the kernel-argument segment, like ViewArgs
using GatherArgs = madrona::mwhip::PlanBatch<GatherPlan, MWHIP_MAX_STEP_GATHERS>;

using madrona::mwhip::HandleSource;
using madrona::mwhip::Resolved;
using madrona::mwhip::cellCopy;
using madrona::mwhip::resolveHandle;
using madrona::mwhip::teamCopy;
using madrona::mwhip::teamZero;

// one wavefront, 64 consecutive handles of one gather
__device__ inline void gatherWave(const GatherPlan *plan, uint32_t item, uint32_t lane)
{
    const uint32_t num_handles = plan->numHandles;
    const uint32_t first = item * 64u;
    const uint32_t in_wave = num_handles - first < 64u ? num_handles - first : 64u;
    const uint32_t i = first + lane;
    const bool valid = lane < in_wave;

    // steps 1 and 2 of the header comment (entity_resolve.hpp)
    const EcsState *S = plan->state;
    const Resolved r = resolveHandle(S, plan->source, i, valid);
    if (valid) {
        plan->archetypes[i] = r.archetype;
        plan->worlds[i] = r.world;
    }

    void *const *col_ptrs = S->colPtr;
    const uint32_t num_slots = S->numComponentSlots;
    const uint32_t num_columns = plan->numColumns;
    for (uint32_t c = 0; c < num_columns; c++) {
        const GatherPlanColumn col = plan->columns[c];
        const uint32_t cell = col.cellBytes;
        const uint32_t T = col.teamLanes;

        // this lane's cell: null when its handle names nothing or the table
        // has no column of the component
        const char *mine = nullptr;
        if (r.archetype >= 0) {
            const char *base =
                (const char *)col_ptrs[(uint64_t)(uint32_t)r.archetype * num_slots + col.component];
            if (base != nullptr) mine = base + (uint64_t)(uint32_t)r.row * cell;
        }
        char *dst = col.dst + (uint64_t)first * cell;

        if (T == 1u) {
            if (valid) {
                char *d = dst + (uint64_t)lane * cell;
                if (mine != nullptr) {
                    cellCopy(d, mine, cell);
                } else {
                    teamZero(d, cell, 0u, 1u);
                }
            }
            continue;
        }
        const uint32_t per_pass = 64u / T;
        const uint32_t t = lane & (T - 1u);
        for (uint32_t pass = 0; pass < T; pass++) {
            const uint32_t owner = pass * per_pass + lane / T;      // < 64
            // (every lane takes part in the cross-lane read)
            const uint64_t from = __shfl((unsigned long long)(uint64_t)mine, (int)owner, 64);
            if (owner < in_wave) {
                char *d = dst + (uint64_t)owner * cell;
                if (from != 0ull) {
                    teamCopy(d, (const char *)from, cell, t, T);
                } else {
                    teamZero(d, cell, t, T);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(kGatherThreads)
entityGatherKernel(GatherArgs args)
{
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t total = madrona::mwhip::batchItems(args);
    for (uint32_t item = blockIdx.x * kGatherWaves + wave; item < total;
         item += gridDim.x * kGatherWaves) {
        // the gather this item belongs to
        uint32_t rel;
        const GatherPlan *plan = madrona::mwhip::planOfItem(args, item, &rel);
        if (plan != nullptr) {
            gatherWave(plan, rel, lane);
        }
    }
}

}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct mwhip_gather_rec {
    uint64_t handle = 0;
    uint32_t numHandles = 0;
    uint32_t items = 0;         // wavefront work items
    uint32_t rowBytes = 0;      // of the listed cells
    std::vector<uint32_t> cellBytes;
    std::vector<char *> buffers;    // into bufDev
    int32_t *archetypesDev = nullptr;
    int32_t *worldsDev = nullptr;
    GatherPlan *planDev = nullptr;
    char *bufDev = nullptr;     // the buffers (256-byte aligned each), archetype, world

    ~mwhip_gather_rec()
    {
        if (planDev != nullptr) (void)hipFree(planDev);
        if (bufDev != nullptr) (void)hipFree(bufDev);
    }
};

namespace {

mwhip_gather_rec *findGather(mwhip_exec *exec, uint64_t handle)
{
    return findObject(exec != nullptr ? &exec->gathers : nullptr, handle);
}

dim3 gatherGrid(mwhip_exec *exec, uint32_t items)
{
    return waveGrid(exec, items, kGatherWaves, 16u);
}

int queueGather(mwhip_exec *exec, mwhip_gather_rec &gather)
{
    return queueBatch(exec, (const void *)&entityGatherKernel, gatherGrid(exec, gather.items),
                      kGatherThreads, singleBatch<GatherArgs>(gather));
}

int computeGather(mwhip_exec *exec, uint64_t handle, bool wait)
{
    return computeObject(exec, findGather(exec, handle), "gather", handle, wait, queueGather);
}

// Bytes the step gathers' last run read: per handle the handle itself, and for
// those that named an entity its slot, its row's Entity and WorldID cells and
// the listed cells (all of them: a table without the column is the exception)
// (KernelLaunch::measuredBytes).
int stepGatherReadBytes(mwhip_exec *exec, double *out)
{
    *out = 0;
    std::vector<int32_t> archetypes;
    for (uint64_t handle : exec->extras.stepGathers) {
        mwhip_gather_rec *gather = findGather(exec, handle);
        if (gather == nullptr) continue;
        archetypes.resize(gather->numHandles);
        HIPCHK(hipMemcpy(archetypes.data(), gather->archetypesDev,
                         archetypes.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        double named = 0;
        for (int32_t a : archetypes) named += a >= 0 ? 1.0 : 0.0;
        *out += (double)gather->numHandles * 8.0 +
            named * ((double)sizeof(EntitySlot) + 12.0 + gather->rowBytes);
    }
    return 0;
}

}

// Tail stage: the ONE launch that recomputes every step gather inside a step
// replay, behind the step views (a gather may read a step view's slab of the
// same replay); none when no step gather is set.
MWHIP_RT int stepGatherStage(mwhip_exec *exec, const LaunchGraph &lg,
                             std::vector<KernelLaunch> &out)
{
    if (lg.isRender) return 0;
    GatherArgs args {};
    double written = 0;
    const uint32_t items = collectStepBatch(
        exec->extras.stepGathers, exec->gathers, args, [&](const mwhip_gather_rec &gather) {
            written += (double)gather.numHandles * ((double)gather.rowBytes + 8.0);
        });
    if (args.num_plans == 0) return 0;
    // (what the step gathers read: from the archetypes they just left)
    out.push_back(stageLaunch((const void *)&entityGatherKernel, gatherGrid(exec, items),
                              kGatherThreads, args, "gather", "gather", written,
                              &stepGatherReadBytes));
    return 0;
}

// What mwhip_gather_create and mwhip_scatter_create refuse about a source and
// a component list, before anything is allocated (`what`: the entry point, in
// front of the text).
MWHIP_RT int checkHandleRequest(mwhip_exec *exec, const char *what,
                                const mwhip_gather_source *source,
                                const uint32_t *component_ids, uint32_t n, const void *out)
{
    if (exec == nullptr || !exec->stateBuilt || out == nullptr) {
        return fail(-2, "%s: no executor state", what);
    }
    if (source == nullptr || source->src == nullptr) {
        return fail(-2, "%s: no source (src == NULL)", what);
    }
    if (((uint64_t)source->src & 3ull) != 0ull || source->record_bytes % 4u != 0u ||
            source->first_byte % 4u != 0u) {
        return fail(-2, "%s: src %p, record_bytes %u and first_byte %u must be "
                    "multiples of 4", what, source->src, source->record_bytes,
                    source->first_byte);
    }
    if (source->handles_per_record == 0u) {
        return fail(-2, "%s: handles_per_record == 0", what);
    }
    if ((uint64_t)source->first_byte + 8ull * source->handles_per_record >
            (uint64_t)source->record_bytes) {
        return fail(-2, "%s: %u handles from byte %u do not fit a record of %u bytes", what,
                    source->handles_per_record, source->first_byte, source->record_bytes);
    }
    if (source->num_records == 0ull) {
        return fail(-2, "%s: num_records == 0", what);
    }
    if (source->num_records > 0x7FFFFFFFull / source->handles_per_record) {
        return fail(-2, "%s: %llu records x %u handles is more than %u handles", what,
                    (unsigned long long)source->num_records, source->handles_per_record,
                    0x7FFFFFFFu);
    }
    if (n > MWHIP_GATHER_MAX_COLUMNS) {
        return fail(-2, "%s: %u components (at most %u)", what, n,
                    (uint32_t)MWHIP_GATHER_MAX_COLUMNS);
    }
    if (n != 0u && component_ids == nullptr) {
        return fail(-2, "%s: %u components and no list", what, n);
    }
    for (uint32_t p = 0; p < n; p++) {
        const uint32_t component = component_ids[p];
        if (component >= exec->components.size() || !exec->components[component].registered ||
                component >= exec->hostState.numComponentSlots) {
            return fail(-2, "%s: column %u: component %u is not registered", what, p,
                        component);
        }
        for (uint32_t q = 0; q < p; q++) {
            if (component_ids[q] == component) {
                return fail(-2, "%s: component %u is listed twice (positions %u "
                            "and %u)", what, component, q, p);
            }
        }
    }
    return 0;
}

extern "C" int mwhip_gather_create(mwhip_exec *exec, const mwhip_gather_source *source,
                                   const uint32_t *component_ids, uint32_t n,
                                   uint64_t *gather_out)
{
    carryStale(exec);
    // (every refusal comes before anything is allocated)
    int rc = checkHandleRequest(exec, "gather_create", source, component_ids, n, gather_out);
    if (rc != 0) return rc;

    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    std::unique_ptr<mwhip_gather_rec> gather(new mwhip_gather_rec {});
    const uint32_t num_handles = (uint32_t)(source->num_records * source->handles_per_record);
    gather->numHandles = num_handles;
    gather->items = (num_handles + 63u) / 64u;

    // the buffers, 256-byte aligned each, then archetype and world
    std::vector<uint64_t> offsets(n);
    uint64_t total = 0;
    for (uint32_t p = 0; p < n; p++) {
        const uint32_t cell = exec->components[component_ids[p]].bytes;
        gather->cellBytes.push_back(cell);
        gather->rowBytes += cell;
        offsets[p] = total;
        total += ((uint64_t)num_handles * cell + 255ull) & ~255ull;
    }
    const uint64_t ints = ((uint64_t)num_handles * sizeof(int32_t) + 255ull) & ~255ull;
    const uint64_t archetypes_at = total;
    const uint64_t worlds_at = total + ints;
    total += 2ull * ints;

    bool ok = hipMalloc((void **)&gather->bufDev, total) == hipSuccess &&
        hipMalloc((void **)&gather->planDev, sizeof(GatherPlan)) == hipSuccess &&
        hipMemset(gather->bufDev, 0, total) == hipSuccess;
    if (ok) {
        gather->archetypesDev = (int32_t *)(gather->bufDev + archetypes_at);
        gather->worldsDev = (int32_t *)(gather->bufDev + worlds_at);
        GatherPlan plan {};
        plan.state = exec->stateDev;
        plan.source = { (const char *)source->src, source->record_bytes, source->first_byte,
                        source->handles_per_record, 0u };
        plan.archetypes = gather->archetypesDev;
        plan.worlds = gather->worldsDev;
        plan.numHandles = num_handles;
        plan.numColumns = n;
        for (uint32_t p = 0; p < n; p++) {
            const uint32_t cell = gather->cellBytes[p];
            uint32_t team = 1;
            while (team < 64u && team * 16u < cell) team <<= 1;
            gather->buffers.push_back(gather->bufDev + offsets[p]);
            plan.columns[p] = { gather->buffers[p], component_ids[p], cell, team, 0u };
        }
        ok = hipMemcpy(gather->planDev, &plan, sizeof(plan), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        return CREATE_FAILED(gather, "gather_create: no device memory for the plan and %llu "
                             "bytes (%u handles)", (unsigned long long)total, num_handles);
    }
    *gather_out = exec->gathers.insert(std::move(gather));
    return 0;
}

extern "C" int mwhip_set_step_gather(mwhip_exec *exec, uint64_t gather, int on)
{
    carryStale(exec);
    if (findGather(exec, gather) == nullptr) return unknownObject("gather", gather);
    return toggleStepSet(exec, &ReplayExtras::stepGathers, gather, on, MWHIP_MAX_STEP_GATHERS,
                         "set_step_gather", "step gathers");
}

extern "C" void mwhip_gather_destroy(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    destroyStepObject(exec, &mwhip_exec::gathers, handle, &mwhip_set_step_gather);
}

extern "C" int mwhip_gather_compute(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeGather(exec, handle, true);
}

extern "C" int mwhip_gather_compute_async(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeGather(exec, handle, false);
}

extern "C" void *mwhip_gather_buffer(mwhip_exec *exec, uint64_t handle, uint32_t column,
                                     uint64_t *bytes_out, uint32_t *cell_bytes_out)
{
    mwhip_gather_rec *gather = findGather(exec, handle);
    if (gather == nullptr) {
        (void)unknownObject("gather", handle);
        return nullptr;
    }
    if (column >= gather->buffers.size()) {
        (void)fail(-2, "gather_buffer: column %u of %u", column,
                   (uint32_t)gather->buffers.size());
        return nullptr;
    }
    if (bytes_out != nullptr) {
        *bytes_out = (uint64_t)gather->numHandles * gather->cellBytes[column];
    }
    if (cell_bytes_out != nullptr) *cell_bytes_out = gather->cellBytes[column];
    return gather->buffers[column];
}

extern "C" int32_t *mwhip_gather_archetypes(mwhip_exec *exec, uint64_t handle)
{
    mwhip_gather_rec *gather = findGather(exec, handle);
    if (gather == nullptr) {
        (void)unknownObject("gather", handle);
        return nullptr;
    }
    return gather->archetypesDev;
}

extern "C" int32_t *mwhip_gather_worlds(mwhip_exec *exec, uint64_t handle)
{
    mwhip_gather_rec *gather = findGather(exec, handle);
    if (gather == nullptr) {
        (void)unknownObject("gather", handle);
        return nullptr;
    }
    return gather->worldsDev;
}
