// libmadrona_hip.so -- world writes: the inverse of a world view.  Padded
// world-major tensors [worlds][max_rows][cell bytes] per listed column, plus an
// int32 take per world, are scattered into the rows of chosen columns of one
// table, where the table is (mwhip_write_*, include/mwhip.h; DESIGN.md §26;
// madrona_amd/write_ref.py is the definition).
//
// A write owns a device-resident PLAN -- the table header, per column the header
// slot its base address is read from (the sort swaps a column with its twin),
// the cell bytes and the column's slab -- and one allocation that holds the
// slabs (the layout of a view of the same columns and max_rows), take and
// count.  Row counts, the sorted prefix and column bases are read on the device
// when the kernel runs: no host round trip, and a plan made before a table grew
// is still right after.
//   worldWriteKernel  a TEAM of T = min(64, next power of two >= max_rows) lanes
//                     owns one world, a wavefront 64 / T consecutive worlds;
//                     wavefronts stride over the (write, 64 / T worlds) items of
//                     up to MWHIP_MAX_STEP_WRITES writes passed by value.
// A team, with k = min(max(take[w], 0), max_rows),
//   1. reads the WorldID cells of its world's range of the sorted prefix
//      ([worldOffsets[w], +worldCounts[w]) clipped to [0, sortedRows)) and
//      counts those equal to w;
//   2. if all of them are: copies min(k, live) rows of each column as ONE byte
//      range from the slab to the table (16, 4 or 1 byte wide by the agreement of
//      the two addresses, with a peeled head: teamCopy); if not (rows destroyed
//      in place): goes through the range again, a row per lane, rank = live
//      rows before it, and writes the rows of rank < k;
//   3. scans the WorldID cells of [sortedRows, numRows) in order and goes on
//      with the ranks behind the prefix rows, a row per lane;
//   4. stores count[w] (every row found, not clipped) with one plain store.
//
// SAFETY.  A table row is written only if its OWN WorldID cell, read in this
// launch, equals w, with w < numWorlds and the row's rank below k <= max_rows:
// step 2's byte range covers rows [lo, lo + min(k, live)) only after step 1 has
// found every cell of [lo, hi) equal to w, and every other write is guarded by
// the test of the row's own cell.  worldOffsets / worldCounts / sortedRows only
// say where to look (teamRange clips them to 0 <= lo <= hi <= prefix <= numRows),
// so a stale or torn header can make a team miss rows, never write rows of
// another world, destroyed rows (WorldID -1) or rows past numRows.  The slab
// index is w * max_rows + rank < numWorlds * max_rows.  A row has one WorldID, so
// teams write disjoint rows; the kernel never writes the WorldID column it reads
// (mwhip_write_create refuses Entity and WorldID), so no team's test depends on
// another's stores.  Nothing but listed cells and count[w] is stored: not the
// header, not the slabs, not take.  No atomics, no spin-waits, no LDS, and no
// workgroup waits for another.
// COST.  Every team scans all of [sortedRows, numRows): worlds x tail / 64
// wavefront iterations, inherited from the view (§23) and like there nothing on
// a table whose rows are all in the prefix, which is the state between steps.
#include "exec_internal.hpp"
#include "world_team.hpp"

namespace {

constexpr uint32_t kWriteThreads = 256;
constexpr uint32_t kWriteWaves = kWriteThreads / 64u;

struct WritePlanColumn {
    void *const *slot;      // &hdr->columns[c] on the device
    const char *src;        // [numWorlds][maxRows][cellBytes]
    uint32_t cellBytes;
    uint32_t pad_;
};

struct WritePlan {
    const TableHdr *hdr;    // on the device
    const int32_t *take;    // [numWorlds]
    int32_t *counts;        // [numWorlds]
    uint32_t numWorlds;
    uint32_t maxRows;
    uint32_t numColumns;
    uint32_t teamLanes;     // T: a power of two, 1 .. 64
    WritePlanColumn columns[MWHIP_WRITE_MAX_COLUMNS];
};

// by value in the kernel-argument segment, like ViewArgs
using WriteArgs = madrona::mwhip::PlanBatch<WritePlan, MWHIP_MAX_STEP_WRITES>;

using madrona::mwhip::cellCopy;
using madrona::mwhip::teamCopy;
using madrona::mwhip::TeamRange;
using madrona::mwhip::teamRange;

// Rows [from, to) of the table, T at a time: those whose WorldID cell is w take
// the ranks behind the `have` rows found before, and those of rank < k get their
// listed cells from world w's slabs.  from, to, w, have and k are the same in
// every lane of a team.  Returns the rows found.
__device__ inline uint32_t teamRows(const WritePlan *plan, const int32_t *world_col,
                                    int32_t from, int32_t to, uint32_t w, uint32_t have,
                                    uint32_t k, uint32_t t, uint32_t T, uint32_t team_shift,
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
        if (is && rank < k) {
            const uint64_t in_row = (uint64_t)w * max_rows + rank;
            for (uint32_t c = 0; c < num_columns; c++) {
                const WritePlanColumn col = plan->columns[c];
                char *dst = (char *)*col.slot;
                cellCopy(dst + (uint64_t)(uint32_t)r * col.cellBytes,
                         col.src + in_row * col.cellBytes, col.cellBytes);
            }
        }
        found += (uint32_t)__builtin_popcountll(m);
    }
    return found;
}

// one wavefront, 64 / T consecutive worlds of one write
__device__ inline void writeWave(const WritePlan *plan, uint32_t item, uint32_t lane)
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
    const TeamRange range = teamRange(plan->hdr, w, valid);
    const int32_t lo = range.lo, hi = range.hi;
    const int32_t *world_col = range.worldCol;

    // rows to write: none of a world that does not exist
    uint32_t k = 0;
    if (valid) {
        const int32_t take = plan->take[w];
        k = take > 0 ? ((uint32_t)take < max_rows ? (uint32_t)take : max_rows) : 0u;
    }

    // 1. the live rows of the range
    uint32_t live = 0;
    for (int32_t base = lo; base < hi; base += (int32_t)T) {
        const int32_t r = base + (int32_t)t;
        const bool is = r < hi && world_col[r] == (int32_t)w;
        live += (uint32_t)__builtin_popcountll((__ballot(is) >> team_shift) & team_bits);
    }

    // 2. write them
    if (live == (uint32_t)(hi - lo)) {
        const uint32_t rows = live < k ? live : k;
        if (rows != 0u) {
            for (uint32_t c = 0; c < num_columns; c++) {
                const WritePlanColumn col = plan->columns[c];
                char *dst = (char *)*col.slot;
                teamCopy(dst + (uint64_t)(uint32_t)lo * col.cellBytes,
                         col.src + (uint64_t)w * max_rows * col.cellBytes,
                         (uint64_t)rows * col.cellBytes, t, T);
            }
        }
    } else {
        (void)teamRows(plan, world_col, lo, hi, w, 0u, k, t, T, team_shift, team_bits);
    }

    // 3. the rows behind the prefix (decided here, per table, from the header)
    // 4. the count
    if (valid) {
        const uint32_t count = live + teamRows(plan, world_col, range.prefix, range.n, w, live,
                                               k, t, T, team_shift, team_bits);
        if (t == 0u) {
            plan->counts[w] = (int32_t)count;
        }
    }
}

__global__ void __launch_bounds__(kWriteThreads)
worldWriteKernel(WriteArgs args)
{
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t total = madrona::mwhip::batchItems(args);
    for (uint32_t item = blockIdx.x * kWriteWaves + wave; item < total;
         item += gridDim.x * kWriteWaves) {
        // the write this item belongs to
        uint32_t rel;
        const WritePlan *plan = madrona::mwhip::planOfItem(args, item, &rel);
        if (plan != nullptr) {
            writeWave(plan, rel, lane);
        }
    }
}

}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct mwhip_write_rec {
    uint64_t handle = 0;
    uint32_t numWorlds = 0;
    uint32_t maxRows = 0;
    uint32_t items = 0;         // wavefront work items
    uint32_t rowBytes = 0;      // of the listed cells
    std::vector<uint32_t> cellBytes;
    std::vector<char *> slabs;  // into bufDev
    int32_t *takeDev = nullptr;
    int32_t *countsDev = nullptr;
    WritePlan *planDev = nullptr;
    char *bufDev = nullptr;     // the slabs (256-byte aligned each), take, the counts

    ~mwhip_write_rec()
    {
        if (planDev != nullptr) (void)hipFree(planDev);
        if (bufDev != nullptr) (void)hipFree(bufDev);
    }
};

namespace {

mwhip_write_rec *findWrite(mwhip_exec *exec, uint64_t handle)
{
    return findObject(exec != nullptr ? &exec->writes : nullptr, handle);
}

dim3 writeGrid(mwhip_exec *exec, uint32_t items)
{
    return waveGrid(exec, items, kWriteWaves, 16u);
}

int queueWrite(mwhip_exec *exec, mwhip_write_rec &write)
{
    return queueBatch(exec, (const void *)&worldWriteKernel, writeGrid(exec, write.items),
                      kWriteThreads, singleBatch<WriteArgs>(write));
}

int applyWrite(mwhip_exec *exec, uint64_t handle, bool wait)
{
    return computeObject(exec, findWrite(exec, handle), "write", handle, wait, queueWrite);
}

// Bytes the step writes' last run moved: the listed cells of the rows it wrote,
// read from the slab and written to the table, and the WorldID cells of the
// rows it counted (KernelLaunch::measuredBytes).
int stepWriteBytes(mwhip_exec *exec, double *out)
{
    *out = 0;
    std::vector<int32_t> counts, take;
    for (uint64_t handle : exec->extras.stepWrites) {
        mwhip_write_rec *write = findWrite(exec, handle);
        if (write == nullptr) continue;
        counts.resize(write->numWorlds);
        take.resize(write->numWorlds);
        HIPCHK(hipMemcpy(counts.data(), write->countsDev, counts.size() * sizeof(int32_t),
                         hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(take.data(), write->takeDev, take.size() * sizeof(int32_t),
                         hipMemcpyDeviceToHost));
        for (uint32_t w = 0; w < write->numWorlds; w++) {
            const double rows = (double)std::max(counts[w], 0);
            const double written = std::min(std::min((double)std::max(take[w], 0), rows),
                                            (double)write->maxRows);
            *out += written * write->rowBytes * 2.0 + rows * 4.0;
        }
    }
    return 0;
}

}

// Head stage: the ONE launch that applies every step write inside a step
// replay, behind the input rings and in front of the first task-graph node;
// none when no step write is set.
MWHIP_RT int stepWriteStage(mwhip_exec *exec, const LaunchGraph &lg,
                            std::vector<KernelLaunch> &out)
{
    if (lg.isRender) return 0;
    WriteArgs args {};
    const uint32_t items = collectStepBatch(exec->extras.stepWrites, exec->writes, args,
                                            [](const mwhip_write_rec &) {});
    if (args.num_plans == 0) return 0;
    // (what the step writes moved: from take and the counts they just left)
    out.push_back(stageLaunch((const void *)&worldWriteKernel, writeGrid(exec, items),
                              kWriteThreads, args, "write", "write", 0.0, &stepWriteBytes));
    return 0;
}

extern "C" int mwhip_write_create(mwhip_exec *exec, uint32_t archetype_id,
                                  const uint32_t *component_ids, uint32_t n,
                                  uint32_t max_rows, uint64_t *write_out)
{
    carryStale(exec);
    // (every refusal comes before anything is allocated)
    if (exec == nullptr || !exec->stateBuilt || write_out == nullptr) {
        return fail(-2, "write_create: no executor state");
    }
    if (n == 0 || component_ids == nullptr) {
        return fail(-2, "write_create: no columns (n == 0)");
    }
    if (n > MWHIP_WRITE_MAX_COLUMNS) {
        return fail(-2, "write_create: %u columns (at most %u)", n,
                    (uint32_t)MWHIP_WRITE_MAX_COLUMNS);
    }
    if (max_rows == 0) {
        return fail(-2, "write_create: max_rows == 0");
    }
    std::vector<mwhip_digest_column> listed(n);
    for (uint32_t p = 0; p < n; p++) {
        listed[p] = { archetype_id, component_ids[p] };
    }
    std::vector<ResolvedColumn> columns;
    int rc = resolveColumns(exec, "write_create", listed.data(), n, columns);
    if (rc != 0) return rc;
    for (uint32_t p = 0; p < n; p++) {
        // (rows are found by their WorldID cell and owned through their Entity
        // cell: neither is a caller's to set)
        if (columns[p].column == 0 || columns[p].column == 1) {
            return fail(-2, "write_create: column %u: component %u is the table's %s column, "
                        "which a write may not list", p, component_ids[p],
                        columns[p].column == 0 ? "Entity" : "WorldID");
        }
    }

    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    std::unique_ptr<mwhip_write_rec> write(new mwhip_write_rec {});
    write->numWorlds = exec->cfg.num_worlds;
    write->maxRows = max_rows;
    uint32_t team = 1;
    while (team < 64u && team < max_rows) team <<= 1;
    const uint32_t per_wave = 64u / team;
    write->items = (write->numWorlds + per_wave - 1u) / per_wave;

    // the slabs, 256-byte aligned each (a view's layout), then take, then the counts
    std::vector<uint64_t> offsets(n);
    uint64_t total = 0;
    for (uint32_t p = 0; p < n; p++) {
        const uint32_t cell = columns[p].cellBytes;
        write->cellBytes.push_back(cell);
        write->rowBytes += cell;
        offsets[p] = total;
        const uint64_t bytes = (uint64_t)write->numWorlds * max_rows * cell;
        total += (bytes + 255ull) & ~255ull;
    }
    const uint64_t per_world_words = ((uint64_t)write->numWorlds * sizeof(int32_t) + 255ull) & ~255ull;
    const uint64_t take_at = total;
    total += per_world_words;
    const uint64_t counts_at = total;
    total += per_world_words;

    // (all zero: an apply before anything is filled takes no rows)
    bool ok = hipMalloc((void **)&write->bufDev, total) == hipSuccess &&
        hipMalloc((void **)&write->planDev, sizeof(WritePlan)) == hipSuccess &&
        hipMemset(write->bufDev, 0, total) == hipSuccess;
    if (ok) {
        write->takeDev = (int32_t *)(write->bufDev + take_at);
        write->countsDev = (int32_t *)(write->bufDev + counts_at);
        WritePlan plan {};
        plan.hdr = exec->hostState.tables + archetype_id;   // (a device address: never read here)
        plan.take = write->takeDev;
        plan.counts = write->countsDev;
        plan.numWorlds = write->numWorlds;
        plan.maxRows = max_rows;
        plan.numColumns = n;
        plan.teamLanes = team;
        for (uint32_t p = 0; p < n; p++) {
            write->slabs.push_back(write->bufDev + offsets[p]);
            plan.columns[p] = { columns[p].slot, write->slabs[p], write->cellBytes[p], 0u };
        }
        ok = hipMemcpy(write->planDev, &plan, sizeof(plan), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        return CREATE_FAILED(write, "write_create: no device memory for the plan and %llu "
                             "bytes (%u worlds x %u rows)", (unsigned long long)total,
                             exec->cfg.num_worlds, max_rows);
    }
    *write_out = exec->writes.insert(std::move(write));
    return 0;
}

extern "C" int mwhip_set_step_write(mwhip_exec *exec, uint64_t write, int on)
{
    carryStale(exec);
    if (findWrite(exec, write) == nullptr) return unknownObject("write", write);
    return toggleStepSet(exec, &ReplayExtras::stepWrites, write, on, MWHIP_MAX_STEP_WRITES,
                         "set_step_write", "step writes");
}

extern "C" void mwhip_write_destroy(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    destroyStepObject(exec, &mwhip_exec::writes, handle, &mwhip_set_step_write);
}

extern "C" int mwhip_write_apply(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return applyWrite(exec, handle, true);
}

extern "C" int mwhip_write_apply_async(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return applyWrite(exec, handle, false);
}

extern "C" void *mwhip_write_buffer(mwhip_exec *exec, uint64_t handle, uint32_t column,
                                    uint64_t *bytes_out, uint32_t *cell_bytes_out)
{
    mwhip_write_rec *write = findWrite(exec, handle);
    if (write == nullptr) {
        (void)unknownObject("write", handle);
        return nullptr;
    }
    if (column >= write->slabs.size()) {
        (void)fail(-2, "write_buffer: column %u of %u", column, (uint32_t)write->slabs.size());
        return nullptr;
    }
    if (bytes_out != nullptr) {
        *bytes_out = (uint64_t)write->numWorlds * write->maxRows * write->cellBytes[column];
    }
    if (cell_bytes_out != nullptr) *cell_bytes_out = write->cellBytes[column];
    return write->slabs[column];
}

extern "C" int32_t *mwhip_write_take(mwhip_exec *exec, uint64_t handle)
{
    mwhip_write_rec *write = findWrite(exec, handle);
    if (write == nullptr) {
        (void)unknownObject("write", handle);
        return nullptr;
    }
    return write->takeDev;
}

extern "C" int32_t *mwhip_write_counts(mwhip_exec *exec, uint64_t handle)
{
    mwhip_write_rec *write = findWrite(exec, handle);
    if (write == nullptr) {
        (void)unknownObject("write", handle);
        return nullptr;
    }
    return write->countsDev;
}
