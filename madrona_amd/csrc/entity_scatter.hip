// libmadrona_hip.so -- entity scatters: the batched ctx.get<T>(e) = v.  N entity
// handles read from device memory, an int32 select per handle and, per listed
// component, a buffer of N cells; an apply stores cell i into the entity handle
// i names, and among selected handles that name the same entity the highest
// index wins (mwhip_scatter_*, include/mwhip.h; DESIGN.md §32;
// madrona_amd/scatter_ref.py is the definition).  The other direction of an
// entity gather (entity_gather.hip), with its source format and its handle
// checks (entity_resolve.hpp).
//
// A scatter owns a device-resident PLAN -- where the handles are, per listed
// component its id, its cell bytes and its input buffer -- and one allocation
// that holds the buffers, select, the three int32 outputs and a CLAIM TABLE:
// slots = the power of two >= 2N, uint32 keys[slots] (entity id + 1, 0: empty)
// and uint32 best[slots] (handle index + 1).  It is keyed by entity ID: two
// handles that pass the generation check with one id name one entity.  It is
// sized by N alone, so the entity store may grow.  Everything about the ECS is
// read on the device when the kernels run, as for a gather.
// Three launches, ordered by the stream or the graph, each over up to
// MWHIP_MAX_STEP_SCATTERS scatters passed by value:
//   scatterZeroKernel   clears every claim table, 16 bytes per lane;
//   scatterClaimKernel  a wavefront owns 64 consecutive handles, a lane one: it
//                       resolves its handle, stores archetype and world, and if
//                       the handle is selected and names an entity, finds or
//                       inserts the id by linear probing from a multiplicative
//                       hash (a compare-and-swap on keys; at most N keys in
//                       >= 2N slots, so an empty slot exists and the loop, which
//                       is bounded by slots, ends there at the latest) and does
//                       atomicMax(best[slot], i + 1).  It keeps nothing else;
//   scatterWriteKernel  resolves again (the tables have not changed in
//                       between), finds its slot with plain loads, stores
//                       written[i] = (best[slot] == i + 1), and the wave copies
//                       the winners' cells from the buffers to the table with
//                       lane teams, as the gather copies the other way: T = the
//                       power of two >= ceil(cell bytes / 16), at most 64, lanes
//                       per cell, the owner lane's destination pointer fetched
//                       with a cross-lane read.  The column's base comes from
//                       colPtr[archetype * numComponentSlots + component]; null
//                       (the table has no such column) is skipped.
//
// SAFETY.  A cell is stored only behind the full resolution of its own handle in
// the same launch (entity_resolve.hpp: 0 <= id < entityCapacity, the slot's
// generation, a registered archetype, 0 <= row < numRows, the row's own Entity
// cell equal to the handle, its WorldID cell not -1), at colPtr's base of that
// archetype + row * cell bytes.  mwhip_scatter_create refuses Entity and WorldID,
// so the kernels never write the columns they read.  Distinct entities have
// distinct rows and one entity has one winner (best[slot] holds one index, the
// ids of a slot's claimants are equal, and step scatters list disjoint
// components), so no two lanes store to the same byte and no lane's test depends
// on another's stores.  Claim-table indices are masked to slots - 1.  Nothing
// else is stored but archetype, world and written: not the header, not the
// buffers, not select, not the source.  The claim table needs agent-scope
// atomics on device memory (relaxed: the launch boundary orders them); apart from
// that no LDS, no spin-wait, and no workgroup waits for another.
#include "exec_internal.hpp"
#include "entity_resolve.hpp"
#include "world_team.hpp"

namespace {

constexpr uint32_t kScatterThreads = 256;
constexpr uint32_t kScatterWaves = kScatterThreads / 64u;
// (checkHandleRequest holds a component list to the gather's limit)
static_assert(MWHIP_SCATTER_MAX_COLUMNS == MWHIP_GATHER_MAX_COLUMNS);

struct ScatterPlanColumn {
    const char *src;        // [numHandles][cellBytes]
    uint32_t component;     // < numComponentSlots, neither Entity nor WorldID (create)
    uint32_t cellBytes;
    uint32_t teamLanes;     // T: a power of two, 1 .. 64
    uint32_t pad_;
};

using madrona::mwhip::HandleSource;

struct ScatterPlan {
    const EcsState *state;  // on the device
    HandleSource source;    // numRecords records of the caller's
    const int32_t *select;  // [numHandles]
    int32_t *archetypes;    // [numHandles]
    int32_t *worlds;        // [numHandles]
    int32_t *written;       // [numHandles]
    uint32_t *keys;         // [slots] entity id + 1, 0: empty
    uint32_t *best;         // [slots] handle index + 1; directly behind keys
    uint32_t numHandles;    // N = numRecords * perRecord <= 2^31 - 1
    uint32_t slotShift;     // 32 - log2(slots), 1 .. 31
    uint32_t slotMask;      // slots - 1
    uint32_t numColumns;
    ScatterPlanColumn columns[MWHIP_SCATTER_MAX_COLUMNS];
};

// by value in the kernel-argument segment, like GatherArgs
using ScatterArgs = madrona::mwhip::PlanBatch<ScatterPlan, MWHIP_MAX_STEP_SCATTERS>;

struct ScatterZeroArgs {
    uint32_t numScatters;
    uint32_t vecs[MWHIP_MAX_STEP_SCATTERS];     // 16-byte vectors of keys + best
    uint32_t *tables[MWHIP_MAX_STEP_SCATTERS];  // keys, 256-byte aligned
};

using madrona::mwhip::CopyU4;
using madrona::mwhip::GlobalU32;
using madrona::mwhip::GlobalU4;
using madrona::mwhip::Resolved;
using madrona::mwhip::cellCopy;
using madrona::mwhip::resolveHandle;
using madrona::mwhip::teamCopy;

__global__ void __launch_bounds__(kScatterThreads)
scatterZeroKernel(ScatterZeroArgs args)
{
    const CopyU4 zero = { 0u, 0u, 0u, 0u };
    const uint32_t tid = blockIdx.x * kScatterThreads + threadIdx.x;
    const uint32_t stride = gridDim.x * kScatterThreads;
#pragma unroll
    for (uint32_t g = 0; g < MWHIP_MAX_STEP_SCATTERS; g++) {
        if (g < args.numScatters) {
            GlobalU4 *table = (GlobalU4 *)(uint64_t)args.tables[g];
            const uint32_t vecs = args.vecs[g];
            for (uint32_t i = tid; i < vecs; i += stride) table[i] = zero;
        }
    }
}

// Where the probing for entity `id` starts (Knuth's multiplicative hash: the
// high bits of the product).
__device__ inline uint32_t claimStart(const ScatterPlan *plan, int32_t id)
{
    return (((uint32_t)id + 1u) * 2654435761u) >> plan->slotShift;
}

// one wavefront, 64 consecutive handles of one scatter: launch 2
__device__ inline void claimWave(const ScatterPlan *plan, uint32_t item, uint32_t lane)
{
    const uint32_t i = item * 64u + lane;
    const bool valid = i < plan->numHandles;
    const Resolved r = resolveHandle(plan->state, plan->source, i, valid);
    if (!valid) return;
    plan->archetypes[i] = r.archetype;
    plan->worlds[i] = r.world;
    if (r.archetype < 0 || plan->select[i] == 0) return;

    const uint32_t key = (uint32_t)r.id + 1u;       // id >= 0: never 0
    const uint32_t mask = plan->slotMask;
    uint32_t slot = claimStart(plan, r.id) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++) {
        uint32_t seen = 0u;
        __hip_atomic_compare_exchange_strong(plan->keys + slot, &seen, key, __ATOMIC_RELAXED,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // (seen: what the slot held; 0 means the key is in now)
        if (seen == 0u || seen == key) {
            __hip_atomic_fetch_max(plan->best + slot, i + 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        slot = (slot + 1u) & mask;
    }
}

// one wavefront, 64 consecutive handles of one scatter: launch 3
__device__ inline void writeWave(const ScatterPlan *plan, uint32_t item, uint32_t lane)
{
    const uint32_t num_handles = plan->numHandles;
    const uint32_t first = item * 64u;
    const uint32_t in_wave = num_handles - first < 64u ? num_handles - first : 64u;
    const uint32_t i = first + lane;
    const bool valid = lane < in_wave;

    const EcsState *S = plan->state;
    const Resolved r = resolveHandle(S, plan->source, i, valid);
    bool winner = false;
    if (valid) {
        if (r.archetype >= 0 && plan->select[i] != 0) {
            // the claim put the key in: an empty slot or the end of the loop is
            // met only if it did not, and then nothing is written
            const GlobalU32 *keys = (const GlobalU32 *)(uint64_t)plan->keys;
            const GlobalU32 *best = (const GlobalU32 *)(uint64_t)plan->best;
            const uint32_t key = (uint32_t)r.id + 1u;
            const uint32_t mask = plan->slotMask;
            uint32_t slot = claimStart(plan, r.id) & mask;
            for (uint32_t probe = 0; probe <= mask; probe++) {
                const uint32_t seen = keys[slot];
                if (seen == key) {
                    winner = best[slot] == i + 1u;
                    break;
                }
                if (seen == 0u) break;
                slot = (slot + 1u) & mask;
            }
        }
        plan->written[i] = winner ? 1 : 0;
    }

    void *const *col_ptrs = S->colPtr;
    const uint32_t num_slots = S->numComponentSlots;
    const uint32_t num_columns = plan->numColumns;
    for (uint32_t c = 0; c < num_columns; c++) {
        const ScatterPlanColumn col = plan->columns[c];
        const uint32_t cell = col.cellBytes;
        const uint32_t T = col.teamLanes;

        // this lane's cell in the table: null unless its handle won and the
        // table has a column of the component
        char *mine = nullptr;
        if (winner) {
            char *base =
                (char *)col_ptrs[(uint64_t)(uint32_t)r.archetype * num_slots + col.component];
            if (base != nullptr) mine = base + (uint64_t)(uint32_t)r.row * cell;
        }
        const char *src = col.src + (uint64_t)first * cell;

        if (T == 1u) {
            if (mine != nullptr) cellCopy(mine, src + (uint64_t)lane * cell, cell);
            continue;
        }
        const uint32_t per_pass = 64u / T;
        const uint32_t t = lane & (T - 1u);
        for (uint32_t pass = 0; pass < T; pass++) {
            const uint32_t owner = pass * per_pass + lane / T;      // < 64
            // (every lane takes part in the cross-lane read)
            const uint64_t to = __shfl((unsigned long long)(uint64_t)mine, (int)owner, 64);
            if (to != 0ull) {
                teamCopy((char *)to, src + (uint64_t)owner * cell, cell, t, T);
            }
        }
    }
}

__global__ void __launch_bounds__(kScatterThreads)
scatterClaimKernel(ScatterArgs args)
{
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t total = madrona::mwhip::batchItems(args);
    for (uint32_t item = blockIdx.x * kScatterWaves + wave; item < total;
         item += gridDim.x * kScatterWaves) {
        uint32_t rel;
        const ScatterPlan *plan = madrona::mwhip::planOfItem(args, item, &rel);
        if (plan != nullptr) claimWave(plan, rel, lane);
    }
}

__global__ void __launch_bounds__(kScatterThreads)
scatterWriteKernel(ScatterArgs args)
{
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t total = madrona::mwhip::batchItems(args);
    for (uint32_t item = blockIdx.x * kScatterWaves + wave; item < total;
         item += gridDim.x * kScatterWaves) {
        uint32_t rel;
        const ScatterPlan *plan = madrona::mwhip::planOfItem(args, item, &rel);
        if (plan != nullptr) writeWave(plan, rel, lane);
    }
}

}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct mwhip_scatter_rec {
    uint64_t handle = 0;
    uint32_t numHandles = 0;
    uint32_t items = 0;         // wavefront work items
    uint32_t slots = 0;         // of the claim table
    uint32_t rowBytes = 0;      // of the listed cells
    std::vector<uint32_t> components;
    std::vector<uint32_t> cellBytes;
    std::vector<char *> buffers;    // into bufDev
    int32_t *selectDev = nullptr;
    int32_t *archetypesDev = nullptr;
    int32_t *worldsDev = nullptr;
    int32_t *writtenDev = nullptr;
    uint32_t *claimDev = nullptr;   // keys[slots], best[slots]
    ScatterPlan *planDev = nullptr;
    char *bufDev = nullptr;     // the buffers (256-byte aligned each), select,
                                // archetype, world, written, the claim table

    ~mwhip_scatter_rec()
    {
        if (planDev != nullptr) (void)hipFree(planDev);
        if (bufDev != nullptr) (void)hipFree(bufDev);
    }
};

namespace {

mwhip_scatter_rec *findScatter(mwhip_exec *exec, uint64_t handle)
{
    return findObject(exec != nullptr ? &exec->scatters : nullptr, handle);
}

dim3 scatterGrid(mwhip_exec *exec, uint32_t items)
{
    return waveGrid(exec, items, kScatterWaves, 16u);
}

dim3 zeroGrid(mwhip_exec *exec, uint64_t vecs)
{
    const uint64_t blocks = (vecs + kScatterThreads - 1u) / kScatterThreads;
    return dim3((uint32_t)std::max<uint64_t>(
                    std::min<uint64_t>(blocks, std::max(exec->numCUs, 1u) * 16u), 1u), 1, 1);
}

// What the three launches need of the scatters in `args` (1 ..
// MWHIP_MAX_STEP_SCATTERS of them) besides that batch.
struct ScatterLaunches {
    ScatterZeroArgs zero {};
    ScatterArgs args {};
    uint64_t vecs = 0;          // of the largest claim table
    double claimBytes = 0;      // of the claim tables
    double perHandleBytes = 0;  // N of every scatter

    // (behind the batch, which just took it)
    void take(const mwhip_scatter_rec &scatter)
    {
        const uint32_t g = zero.numScatters;
        zero.vecs[g] = scatter.slots / 2u;      // 2 * slots words of 4 bytes
        zero.tables[g] = scatter.claimDev;
        zero.numScatters += 1;
        vecs = std::max<uint64_t>(vecs, scatter.slots / 2u);
        claimBytes += (double)scatter.slots * 8.0;
        perHandleBytes += (double)scatter.numHandles;
    }
};

int queueScatter(mwhip_exec *exec, mwhip_scatter_rec &scatter)
{
    ScatterLaunches l;
    l.args = singleBatch<ScatterArgs>(scatter);
    l.take(scatter);
    const dim3 grid = scatterGrid(exec, scatter.items);
    int rc = queueBatch(exec, (const void *)&scatterZeroKernel, zeroGrid(exec, l.vecs),
                        kScatterThreads, l.zero);
    if (rc == 0) {
        rc = queueBatch(exec, (const void *)&scatterClaimKernel, grid, kScatterThreads, l.args);
    }
    if (rc == 0) {
        rc = queueBatch(exec, (const void *)&scatterWriteKernel, grid, kScatterThreads, l.args);
    }
    return rc;
}

int applyScatter(mwhip_exec *exec, uint64_t handle, bool wait)
{
    return computeObject(exec, findScatter(exec, handle), "scatter", handle, wait, queueScatter);
}

// What the step scatters' last run left: handles that named an entity and
// handles that won, over every step scatter (the latter weighted by the listed
// cells' bytes).
int stepScatterCounts(mwhip_exec *exec, double *named_out, double *won_bytes_out)
{
    *named_out = 0;
    *won_bytes_out = 0;
    std::vector<int32_t> archetypes, written;
    for (uint64_t handle : exec->extras.stepScatters) {
        mwhip_scatter_rec *scatter = findScatter(exec, handle);
        if (scatter == nullptr) continue;
        archetypes.resize(scatter->numHandles);
        written.resize(scatter->numHandles);
        HIPCHK(hipMemcpy(archetypes.data(), scatter->archetypesDev,
                         archetypes.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(written.data(), scatter->writtenDev,
                         written.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        double won = 0;
        for (int32_t a : archetypes) *named_out += a >= 0 ? 1.0 : 0.0;
        for (int32_t w : written) won += w != 0 ? 1.0 : 0.0;
        *won_bytes_out += won * scatter->rowBytes;
    }
    return 0;
}

// Bytes only the device knows (KernelLaunch::measuredBytes): per handle that
// named an entity its slot and its row's Entity and WorldID cells, in both
// launches that resolve; per winner the listed cells, read from the buffers and
// written to the table (all of them: a table without the column is the exception).
int stepScatterClaimBytes(mwhip_exec *exec, double *out)
{
    double named = 0, won_bytes = 0;
    int rc = stepScatterCounts(exec, &named, &won_bytes);
    *out = named * ((double)sizeof(EntitySlot) + 12.0);
    return rc;
}

int stepScatterWriteBytes(mwhip_exec *exec, double *out)
{
    double named = 0, won_bytes = 0;
    int rc = stepScatterCounts(exec, &named, &won_bytes);
    *out = named * ((double)sizeof(EntitySlot) + 12.0) + 2.0 * won_bytes;
    return rc;
}

}

// Head stage: the THREE launches that apply every step scatter inside a step
// replay, directly behind the step writes and in front of the first task-graph
// node; none when no step scatter is set.
MWHIP_RT int stepScatterStage(mwhip_exec *exec, const LaunchGraph &lg,
                              std::vector<KernelLaunch> &out)
{
    if (lg.isRender) return 0;
    ScatterLaunches l;
    const uint32_t items = collectStepBatch(
        exec->extras.stepScatters, exec->scatters, l.args,
        [&](const mwhip_scatter_rec &scatter) { l.take(scatter); });
    if (l.args.num_plans == 0) return 0;
    const dim3 grid = scatterGrid(exec, items);

    out.push_back(stageLaunch((const void *)&scatterZeroKernel, zeroGrid(exec, l.vecs),
                              kScatterThreads, l.zero, "scatter", "scatter.zero", l.claimBytes));
    // per handle: the handle and select read, archetype and world written
    out.push_back(stageLaunch((const void *)&scatterClaimKernel, grid, kScatterThreads, l.args,
                              "scatter", "scatter.claim", l.perHandleBytes * (8.0 + 4.0 + 8.0),
                              &stepScatterClaimBytes));
    // per handle: the handle and select read, written written
    out.push_back(stageLaunch((const void *)&scatterWriteKernel, grid, kScatterThreads, l.args,
                              "scatter", "scatter.write", l.perHandleBytes * (8.0 + 4.0 + 4.0),
                              &stepScatterWriteBytes));
    return 0;
}

extern "C" int mwhip_scatter_create(mwhip_exec *exec, const mwhip_gather_source *source,
                                    const uint32_t *component_ids, uint32_t n,
                                    uint64_t *scatter_out)
{
    carryStale(exec);
    // (every refusal comes before anything is allocated)
    int rc = checkHandleRequest(exec, "scatter_create", source, component_ids, n, scatter_out);
    if (rc != 0) return rc;
    if (n == 0u) {
        return fail(-2, "scatter_create: no components (n == 0)");
    }
    for (uint32_t p = 0; p < n; p++) {
        // (rows are found through their Entity cell and live by their WorldID
        // cell: neither is a caller's to set)
        if (component_ids[p] == 0u || component_ids[p] == 1u) {
            return fail(-2, "scatter_create: column %u: component %u is the %s component, "
                        "which a scatter may not list", p, component_ids[p],
                        component_ids[p] == 0u ? "Entity" : "WorldID");
        }
    }

    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    std::unique_ptr<mwhip_scatter_rec> scatter(new mwhip_scatter_rec {});
    const uint32_t num_handles = (uint32_t)(source->num_records * source->handles_per_record);
    scatter->numHandles = num_handles;
    scatter->items = (num_handles + 63u) / 64u;
    // the power of two >= 2N (N <= 2^31 - 1: at most 2^32, which a uint32 mask
    // and a shift of 0 would need; 2^31 slots hold N keys as well, if less
    // sparsely, and nobody has memory for either)
    uint32_t log2_slots = 1;
    while (log2_slots < 31u && (1ull << log2_slots) < 2ull * num_handles) log2_slots++;
    scatter->slots = 1u << log2_slots;

    // the buffers, 256-byte aligned each, then select, archetype, world,
    // written, then the claim table
    std::vector<uint64_t> offsets(n);
    uint64_t total = 0;
    for (uint32_t p = 0; p < n; p++) {
        const uint32_t cell = exec->components[component_ids[p]].bytes;
        scatter->components.push_back(component_ids[p]);
        scatter->cellBytes.push_back(cell);
        scatter->rowBytes += cell;
        offsets[p] = total;
        total += ((uint64_t)num_handles * cell + 255ull) & ~255ull;
    }
    const uint64_t ints = ((uint64_t)num_handles * sizeof(int32_t) + 255ull) & ~255ull;
    const uint64_t select_at = total;
    const uint64_t archetypes_at = total + ints;
    const uint64_t worlds_at = total + 2ull * ints;
    const uint64_t written_at = total + 3ull * ints;
    total += 4ull * ints;
    const uint64_t claim_at = total;
    total += (2ull * scatter->slots * sizeof(uint32_t) + 255ull) & ~255ull;

    // (all zero: an apply before anything is filled selects nothing)
    bool ok = hipMalloc((void **)&scatter->bufDev, total) == hipSuccess &&
        hipMalloc((void **)&scatter->planDev, sizeof(ScatterPlan)) == hipSuccess &&
        hipMemset(scatter->bufDev, 0, total) == hipSuccess;
    if (ok) {
        scatter->selectDev = (int32_t *)(scatter->bufDev + select_at);
        scatter->archetypesDev = (int32_t *)(scatter->bufDev + archetypes_at);
        scatter->worldsDev = (int32_t *)(scatter->bufDev + worlds_at);
        scatter->writtenDev = (int32_t *)(scatter->bufDev + written_at);
        scatter->claimDev = (uint32_t *)(scatter->bufDev + claim_at);
        ScatterPlan plan {};
        plan.state = exec->stateDev;
        plan.source = { (const char *)source->src, source->record_bytes, source->first_byte,
                        source->handles_per_record, 0u };
        plan.select = scatter->selectDev;
        plan.archetypes = scatter->archetypesDev;
        plan.worlds = scatter->worldsDev;
        plan.written = scatter->writtenDev;
        plan.keys = scatter->claimDev;
        plan.best = scatter->claimDev + scatter->slots;
        plan.numHandles = num_handles;
        plan.slotShift = 32u - log2_slots;
        plan.slotMask = scatter->slots - 1u;
        plan.numColumns = n;
        for (uint32_t p = 0; p < n; p++) {
            const uint32_t cell = scatter->cellBytes[p];
            uint32_t team = 1;
            while (team < 64u && team * 16u < cell) team <<= 1;
            scatter->buffers.push_back(scatter->bufDev + offsets[p]);
            plan.columns[p] = { scatter->buffers[p], component_ids[p], cell, team, 0u };
        }
        ok = hipMemcpy(scatter->planDev, &plan, sizeof(plan), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        return CREATE_FAILED(scatter, "scatter_create: no device memory for the plan and %llu "
                             "bytes (%u handles)", (unsigned long long)total, num_handles);
    }
    *scatter_out = exec->scatters.insert(std::move(scatter));
    return 0;
}

extern "C" int mwhip_set_step_scatter(mwhip_exec *exec, uint64_t scatter, int on)
{
    carryStale(exec);
    mwhip_scatter_rec *rec = findScatter(exec, scatter);
    if (rec == nullptr) return unknownObject("scatter", scatter);
    // (two step scatters run in the same launches, each with a claim table of
    // its own: on one component they could store to one cell)
    const auto disjoint = [exec, rec, scatter] {
        for (uint64_t other_handle : exec->extras.stepScatters) {
            mwhip_scatter_rec *other = findScatter(exec, other_handle);
            if (other == nullptr) continue;
            for (uint32_t component : rec->components) {
                if (std::find(other->components.begin(), other->components.end(), component) !=
                        other->components.end()) {
                    return fail(-2, "set_step_scatter: scatter %llu lists component %u, which "
                                "step scatter %llu lists already",
                                (unsigned long long)scatter, component,
                                (unsigned long long)other_handle);
                }
            }
        }
        return 0;
    };
    return toggleStepSet(exec, &ReplayExtras::stepScatters, scatter, on, MWHIP_MAX_STEP_SCATTERS,
                         "set_step_scatter", "step scatters", disjoint);
}

extern "C" void mwhip_scatter_destroy(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    destroyStepObject(exec, &mwhip_exec::scatters, handle, &mwhip_set_step_scatter);
}

extern "C" int mwhip_scatter_apply(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return applyScatter(exec, handle, true);
}

extern "C" int mwhip_scatter_apply_async(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return applyScatter(exec, handle, false);
}

extern "C" void *mwhip_scatter_buffer(mwhip_exec *exec, uint64_t handle, uint32_t column,
                                      uint64_t *bytes_out, uint32_t *cell_bytes_out)
{
    mwhip_scatter_rec *scatter = findScatter(exec, handle);
    if (scatter == nullptr) {
        (void)unknownObject("scatter", handle);
        return nullptr;
    }
    if (column >= scatter->buffers.size()) {
        (void)fail(-2, "scatter_buffer: column %u of %u", column,
                   (uint32_t)scatter->buffers.size());
        return nullptr;
    }
    if (bytes_out != nullptr) {
        *bytes_out = (uint64_t)scatter->numHandles * scatter->cellBytes[column];
    }
    if (cell_bytes_out != nullptr) *cell_bytes_out = scatter->cellBytes[column];
    return scatter->buffers[column];
}

namespace {

// one of a scatter's int32 [N] arrays, or NULL with -3's message
int32_t *scatterInts(mwhip_exec *exec, uint64_t handle, int32_t *mwhip_scatter_rec::*which)
{
    mwhip_scatter_rec *scatter = findScatter(exec, handle);
    if (scatter == nullptr) {
        (void)unknownObject("scatter", handle);
        return nullptr;
    }
    return scatter->*which;
}

}

extern "C" int32_t *mwhip_scatter_select(mwhip_exec *exec, uint64_t handle)
{
    return scatterInts(exec, handle, &mwhip_scatter_rec::selectDev);
}

extern "C" int32_t *mwhip_scatter_archetypes(mwhip_exec *exec, uint64_t handle)
{
    return scatterInts(exec, handle, &mwhip_scatter_rec::archetypesDev);
}

extern "C" int32_t *mwhip_scatter_worlds(mwhip_exec *exec, uint64_t handle)
{
    return scatterInts(exec, handle, &mwhip_scatter_rec::worldsDev);
}

extern "C" int32_t *mwhip_scatter_written(mwhip_exec *exec, uint64_t handle)
{
    return scatterInts(exec, handle, &mwhip_scatter_rec::writtenDev);
}
