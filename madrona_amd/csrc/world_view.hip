// libmadrona_hip.so -- world views: a dense, zero-padded, world-major copy of
// chosen columns of one table, [worlds][max_rows][cell bytes] per column plus an
// int32 count per world, written where the table is (mwhip_view_*,
// include/mwhip.h; madrona_amd/view_ref.py is the definition).
//
// A view owns a device-resident PLAN -- the table header, per column the header
// slot its base address is read from (the sort swaps a column with its twin),
// the cell bytes and the column's slab of the view -- and one allocation that
// holds the slabs and the counts.  Row counts, the sorted prefix and column
// bases are read on the device when the kernel runs: no host round trip, and a
// plan made before a table grew is still right after.
//   worldViewKernel   a TEAM of T = min(64, next power of two >= max_rows) lanes
//                     owns one world, a wavefront 64 / T consecutive worlds;
//                     wavefronts stride over the (view, 64 / T worlds) items of
//                     up to MWHIP_MAX_STEP_VIEWS views passed by value.
// A team
//   1. reads the WorldID cells of its world's range of the sorted prefix
//      ([worldOffsets[w], +worldCounts[w]) clipped to [0, sortedRows)) and
//      counts those equal to w;
//   2. if all of them are: copies each column's cells of the range as ONE byte
//      range (they are contiguous in the table and in the view), 16 bytes per
//      lane where source and destination agree modulo 16, dwords where they
//      agree modulo 4, bytes otherwise; if not (rows destroyed in place): goes
//      through the range again, a row per lane, rank = live rows before it
//      (a ballot masked to the team + popcount);
//   3. scans the WorldID cells of [sortedRows, numRows) in order -- nothing
//      when the table has no rows behind its prefix, the whole table when it
//      has no prefix -- and appends the rows of its world, a row per lane;
//   4. zeroes what is left of its slabs and stores count[w].
// A row is placed by its own WorldID cell; worldOffsets / worldCounts /
// sortedRows only say where to look, and every output index is w < numWorlds
// and rank < max_rows by construction.  A team writes nothing but its own
// world's slabs: no atomics, no spin-waits, no workgroup waits for another, no
// LDS.  (copyChunk of copy_chunk.hpp moves a chunk with a whole workgroup; a
// team is a part of a wavefront, so only its vector types are shared.  What a
// team does that the world writes and the entity gathers need too -- teamCopy,
// teamZero, cellCopy, teamRange -- is in world_team.hpp.)
#include "exec_internal.hpp"
#include "world_team.hpp"

namespace {

constexpr uint32_t kViewThreads = 256;
constexpr uint32_t kViewWaves = kViewThreads / 64u;

struct ViewPlanColumn {
    void *const *slot;      // &hdr->columns[c] on the device
    char *dst;              // [numWorlds][maxRows][cellBytes]
    uint32_t cellBytes;
    uint32_t pad_;
};

struct ViewPlan {
    const TableHdr *hdr;    // on the device
    int32_t *counts;        // [numWorlds]
    uint32_t numWorlds;
    uint32_t maxRows;
    uint32_t numColumns;
    uint32_t teamLanes;     // T: a power of two, 1 .. 64
    ViewPlanColumn columns[MWHIP_VIEW_MAX_COLUMNS];
};

// by value in the kernel-argument segment, like OutputRingArgs
using ViewArgs = madrona::mwhip::PlanBatch<ViewPlan, MWHIP_MAX_STEP_VIEWS>;

using madrona::mwhip::CopyU4;
using madrona::mwhip::GlobalU4;
using madrona::mwhip::GlobalU32;
using madrona::mwhip::GlobalU8;
using madrona::mwhip::cellCopy;
using madrona::mwhip::teamCopy;
using madrona::mwhip::teamZero;

// Rows [from, to) of the table, T at a time: those whose WorldID cell is w are
// appended to world w's slabs behind the `have` rows already there (rows past
// maxRows are counted, not copied).  from, to, w and have are the same in every
// lane of a team.  Returns the rows found.
__device__ inline uint32_t teamRows(const ViewPlan *plan, const int32_t *world_col,
                                    int32_t from, int32_t to, uint32_t w, uint32_t have,
                                    uint32_t t, uint32_t T, uint32_t team_shift,
                                    unsigned long long team_bits)
{
    const uint32_t max_rows = plan->maxRows;
    const uint32_t num_columns = plan->numColumns;
    uint32_t found = 0;
    for (int32_t base = from; base < to; base += (int32_t)T) {
        const int32_t r = base + (int32_t)t;
        const bool is = r < to && world_col[r] == (int32_t)w;
        const unsigned long long m = (__ballot(is) >> team_shift) & team_bits;
        const uint32_t rank =
            have + found + (uint32_t)__builtin_popcountll(m & ((1ull << t) - 1ull));
        if (is && rank < max_rows) {
            const uint64_t out_row = (uint64_t)w * max_rows + rank;
            for (uint32_t c = 0; c < num_columns; c++) {
                const ViewPlanColumn col = plan->columns[c];
                const char *src = (const char *)*col.slot;
                cellCopy(col.dst + out_row * col.cellBytes,
                         src + (uint64_t)(uint32_t)r * col.cellBytes, col.cellBytes);
            }
        }
        found += (uint32_t)__builtin_popcountll(m);
    }
    return found;
}

// one wavefront, 64 / T consecutive worlds of one view
__device__ inline void viewWave(const ViewPlan *plan, uint32_t item, uint32_t lane)
{
    const uint32_t T = plan->teamLanes;
    const uint32_t num_worlds = plan->numWorlds;
    const uint32_t max_rows = plan->maxRows;
    const uint32_t num_columns = plan->numColumns;
    const uint32_t team = lane / T;
    const uint32_t t = lane & (T - 1u);
    const uint32_t team_shift = team * T;
    const unsigned long long team_bits = T >= 64u ? ~0ull : (1ull << T) - 1ull;
    const uint32_t w = item * (64u / T) + team;
    const bool valid = w < num_worlds;

    // where world w's rows of the sorted prefix are (a hint: each row is still
    // tested against its own WorldID cell)
    const madrona::mwhip::TeamRange range = madrona::mwhip::teamRange(plan->hdr, w, valid);
    const int32_t n = range.n, prefix = range.prefix, lo = range.lo, hi = range.hi;
    const int32_t *world_col = range.worldCol;

    // 1. the live rows of the range
    uint32_t live = 0;
    for (int32_t base = lo; base < hi; base += (int32_t)T) {
        const int32_t r = base + (int32_t)t;
        const bool is = r < hi && world_col[r] == (int32_t)w;
        live += (uint32_t)__builtin_popcountll((__ballot(is) >> team_shift) & team_bits);
    }

    // 2. copy them
    if (live == (uint32_t)(hi - lo)) {
        const uint32_t k = live < max_rows ? live : max_rows;
        if (k != 0u) {
            for (uint32_t c = 0; c < num_columns; c++) {
                const ViewPlanColumn col = plan->columns[c];
                const char *src = (const char *)*col.slot;
                teamCopy(col.dst + (uint64_t)w * max_rows * col.cellBytes,
                         src + (uint64_t)(uint32_t)lo * col.cellBytes,
                         (uint64_t)k * col.cellBytes, t, T);
            }
        }
    } else {
        (void)teamRows(plan, world_col, lo, hi, w, 0u, t, T, team_shift, team_bits);
    }

    // 3. the rows behind the prefix (decided here, per table, from the header)
    uint32_t count = live;
    if (valid) {
        count += teamRows(plan, world_col, prefix, n, w, live, t, T, team_shift, team_bits);
    }

    // 4. padding and count
    if (valid) {
        const uint32_t k = count < max_rows ? count : max_rows;
        if (k < max_rows) {
            for (uint32_t c = 0; c < num_columns; c++) {
                const ViewPlanColumn col = plan->columns[c];
                teamZero(col.dst + ((uint64_t)w * max_rows + k) * col.cellBytes,
                         (uint64_t)(max_rows - k) * col.cellBytes, t, T);
            }
        }
        if (t == 0u) {
            plan->counts[w] = (int32_t)count;
        }
    }
}

__global__ void __launch_bounds__(kViewThreads)
worldViewKernel(ViewArgs args)
{
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t total = madrona::mwhip::batchItems(args);
    for (uint32_t item = blockIdx.x * kViewWaves + wave; item < total;
         item += gridDim.x * kViewWaves) {
        // the view this item belongs to
        uint32_t rel;
        const ViewPlan *plan = madrona::mwhip::planOfItem(args, item, &rel);
        if (plan != nullptr) {
            viewWave(plan, rel, lane);
        }
    }
}

}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct mwhip_view_rec {
    uint64_t handle = 0;
    uint32_t numWorlds = 0;
    uint32_t maxRows = 0;
    uint32_t items = 0;         // wavefront work items
    uint32_t rowBytes = 0;      // of the listed cells
    std::vector<uint32_t> cellBytes;
    std::vector<char *> slabs;  // into bufDev
    int32_t *countsDev = nullptr;
    ViewPlan *planDev = nullptr;
    char *bufDev = nullptr;     // the slabs (256-byte aligned each), then the counts

    ~mwhip_view_rec()
    {
        if (planDev != nullptr) (void)hipFree(planDev);
        if (bufDev != nullptr) (void)hipFree(bufDev);
    }
};

namespace {

mwhip_view_rec *findView(mwhip_exec *exec, uint64_t handle)
{
    return findObject(exec != nullptr ? &exec->views : nullptr, handle);
}

dim3 viewGrid(mwhip_exec *exec, uint32_t items)
{
    return waveGrid(exec, items, kViewWaves, 16u);
}

int queueView(mwhip_exec *exec, mwhip_view_rec &view)
{
    return queueBatch(exec, (const void *)&worldViewKernel, viewGrid(exec, view.items),
                      kViewThreads, singleBatch<ViewArgs>(view));
}

int computeView(mwhip_exec *exec, uint64_t handle, bool wait)
{
    return computeObject(exec, findView(exec, handle), "view", handle, wait, queueView);
}

// Bytes the step views' last run read: the listed cells of the rows it copied
// and the WorldID cells of the rows it counted (KernelLaunch::measuredBytes).
int stepViewReadBytes(mwhip_exec *exec, double *out)
{
    *out = 0;
    std::vector<int32_t> counts;
    for (uint64_t handle : exec->extras.stepViews) {
        mwhip_view_rec *view = findView(exec, handle);
        if (view == nullptr) continue;
        counts.resize(view->numWorlds);
        HIPCHK(hipMemcpy(counts.data(), view->countsDev, counts.size() * sizeof(int32_t),
                         hipMemcpyDeviceToHost));
        for (int32_t count : counts) {
            const double rows = (double)std::max(count, 0);
            *out += std::min(rows, (double)view->maxRows) * view->rowBytes + rows * 4.0;
        }
    }
    return 0;
}

}

// Tail stage: the ONE launch that recomputes every step view inside a step
// replay; none when no step view is set.
MWHIP_RT int stepViewStage(mwhip_exec *exec, const LaunchGraph &lg,
                           std::vector<KernelLaunch> &out)
{
    if (lg.isRender) return 0;
    ViewArgs args {};
    double written = 0;
    const uint32_t items = collectStepBatch(
        exec->extras.stepViews, exec->views, args, [&](const mwhip_view_rec &view) {
            written += (double)view.numWorlds * ((double)view.maxRows * view.rowBytes + 4.0);
        });
    if (args.num_plans == 0) return 0;
    // (what the step views read: from the counts they just left)
    out.push_back(stageLaunch((const void *)&worldViewKernel, viewGrid(exec, items), kViewThreads,
                              args, "view", "view", written, &stepViewReadBytes));
    return 0;
}

extern "C" int mwhip_view_create(mwhip_exec *exec, uint32_t archetype_id,
                                 const uint32_t *component_ids, uint32_t n,
                                 uint32_t max_rows, uint64_t *view_out)
{
    carryStale(exec);
    // (every refusal comes before anything is allocated)
    if (exec == nullptr || !exec->stateBuilt || view_out == nullptr) {
        return fail(-2, "view_create: no executor state");
    }
    if (n == 0 || component_ids == nullptr) {
        return fail(-2, "view_create: no columns (n == 0)");
    }
    if (n > MWHIP_VIEW_MAX_COLUMNS) {
        return fail(-2, "view_create: %u columns (at most %u)", n,
                    (uint32_t)MWHIP_VIEW_MAX_COLUMNS);
    }
    if (max_rows == 0) {
        return fail(-2, "view_create: max_rows == 0");
    }
    std::vector<mwhip_digest_column> listed(n);
    for (uint32_t p = 0; p < n; p++) {
        listed[p] = { archetype_id, component_ids[p] };
    }
    std::vector<ResolvedColumn> columns;
    int rc = resolveColumns(exec, "view_create", listed.data(), n, columns);
    if (rc != 0) return rc;

    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    std::unique_ptr<mwhip_view_rec> view(new mwhip_view_rec {});
    view->numWorlds = exec->cfg.num_worlds;
    view->maxRows = max_rows;
    uint32_t team = 1;
    while (team < 64u && team < max_rows) team <<= 1;
    const uint32_t per_wave = 64u / team;
    view->items = (view->numWorlds + per_wave - 1u) / per_wave;

    // the slabs, 256-byte aligned each, then the counts
    std::vector<uint64_t> offsets(n);
    uint64_t total = 0;
    for (uint32_t p = 0; p < n; p++) {
        const uint32_t cell = columns[p].cellBytes;
        view->cellBytes.push_back(cell);
        view->rowBytes += cell;
        offsets[p] = total;
        const uint64_t bytes = (uint64_t)view->numWorlds * max_rows * cell;
        total += (bytes + 255ull) & ~255ull;
    }
    const uint64_t counts_at = total;
    total += ((uint64_t)view->numWorlds * sizeof(int32_t) + 255ull) & ~255ull;

    bool ok = hipMalloc((void **)&view->bufDev, total) == hipSuccess &&
        hipMalloc((void **)&view->planDev, sizeof(ViewPlan)) == hipSuccess &&
        hipMemset(view->bufDev, 0, total) == hipSuccess;
    if (ok) {
        view->countsDev = (int32_t *)(view->bufDev + counts_at);
        ViewPlan plan {};
        plan.hdr = exec->hostState.tables + archetype_id;   // (a device address: never read here)
        plan.counts = view->countsDev;
        plan.numWorlds = view->numWorlds;
        plan.maxRows = max_rows;
        plan.numColumns = n;
        plan.teamLanes = team;
        for (uint32_t p = 0; p < n; p++) {
            view->slabs.push_back(view->bufDev + offsets[p]);
            plan.columns[p] = { columns[p].slot, view->slabs[p], view->cellBytes[p], 0u };
        }
        ok = hipMemcpy(view->planDev, &plan, sizeof(plan), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        return CREATE_FAILED(view, "view_create: no device memory for the plan and %llu "
                             "bytes (%u worlds x %u rows)", (unsigned long long)total,
                             exec->cfg.num_worlds, max_rows);
    }
    *view_out = exec->views.insert(std::move(view));
    return 0;
}

extern "C" int mwhip_set_step_view(mwhip_exec *exec, uint64_t view, int on)
{
    carryStale(exec);
    if (findView(exec, view) == nullptr) return unknownObject("view", view);
    return toggleStepSet(exec, &ReplayExtras::stepViews, view, on, MWHIP_MAX_STEP_VIEWS,
                         "set_step_view", "step views");
}

extern "C" void mwhip_view_destroy(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    destroyStepObject(exec, &mwhip_exec::views, handle, &mwhip_set_step_view);
}

extern "C" int mwhip_view_compute(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeView(exec, handle, true);
}

extern "C" int mwhip_view_compute_async(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeView(exec, handle, false);
}

extern "C" void *mwhip_view_buffer(mwhip_exec *exec, uint64_t handle, uint32_t column,
                                   uint64_t *bytes_out, uint32_t *cell_bytes_out)
{
    mwhip_view_rec *view = findView(exec, handle);
    if (view == nullptr) {
        (void)unknownObject("view", handle);
        return nullptr;
    }
    if (column >= view->slabs.size()) {
        (void)fail(-2, "view_buffer: column %u of %u", column, (uint32_t)view->slabs.size());
        return nullptr;
    }
    if (bytes_out != nullptr) {
        *bytes_out = (uint64_t)view->numWorlds * view->maxRows * view->cellBytes[column];
    }
    if (cell_bytes_out != nullptr) *cell_bytes_out = view->cellBytes[column];
    return view->slabs[column];
}

extern "C" int32_t *mwhip_view_counts(mwhip_exec *exec, uint64_t handle)
{
    mwhip_view_rec *view = findView(exec, handle);
    if (view == nullptr) {
        (void)unknownObject("view", handle);
        return nullptr;
    }
    return view->countsDev;
}
