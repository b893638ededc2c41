// libmadrona_hip.so -- executor snapshots: all world state saved into and
// restored from device memory (mwhip_snapshot_*, include/mwhip.h).
//
// The state of a batch of worlds is a few hundred SEGMENTS: every column of
// every table, the tables' row counts and world ranges, the entity slots, the
// id caches, the per-world data, the persistent region and a few header words.
// How long most of them are is known on the device only (numRows, the ids in
// use, persistOffset).  A hipMemcpyAsync per segment costs a launch each and a
// host round trip for the lengths; here one kernel walks a device-resident
// segment table instead:
//   snapshotMeasure  (save only, one workgroup) reads the live lengths, checks
//                    them against the room the snapshot has, and leaves every
//                    segment's byte count and the prefix sums of their 16 KiB
//                    chunks IN THE SNAPSHOT
//   snapshotCopy     (save and restore, numCUs x 8 workgroups) strides over the
//                    (segment, chunk) pairs and moves 16 bytes per lane
// A restore takes its lengths from the snapshot, never from the live headers:
// it overwrites those (numRows is itself a segment), and a workgroup that read
// one would race with the workgroup that writes it.  Column base addresses are
// read from the table headers (the sort swaps a column with its twin; a
// snapshot holds the values of whichever side is current and restores into
// whichever side is current then) -- no kernel of a restore writes them.
// No atomics, no spin-waits: two plain launches on the executor's stream.
#include "exec_internal.hpp"
#include "copy_chunk.hpp"

namespace {

constexpr uint32_t kSnapThreads = kCopyThreads;
constexpr uint32_t kSnapChunk = kCopyChunk;     // bytes per (segment, chunk) pair
constexpr uint64_t kSnapAlign = 256;            // every segment's place in the snapshot

// where a segment's length comes from when it is saved
enum SnapCount : uint32_t {
    kSnapFixed = 0,         // countArg rows
    kSnapTableRows = 1,     // tables[countArg].numRows rows
    kSnapEntities = 2,      // the entity ids in use
    kSnapPersist = 3,       // persistOffset bytes
};

struct SnapSegment {
    void *const *liveSlot;  // where the live base address is read (a table
                            // header's columns[c]: the sort swaps sides), or
    char *live;             // ... the live base itself (liveSlot == nullptr)
    uint64_t savedOffset;   // in the snapshot's data (multiple of kSnapAlign)
    uint64_t roomBytes;     // what the snapshot has room for
    uint32_t bytesPerRow;
    uint32_t countKind;     // SnapCount
    uint32_t countArg;
    uint32_t pad_;
};

// head of a snapshot's device-resident description; behind it
//   uint64_t    bytes[numSegments]         what the last save holds of each
//   uint32_t    chunkStart[numSegments + 1]
//   SnapSegment segments[numSegments]
struct SnapHeader {
    uint32_t numSegments;
    uint32_t saved;         // a save has measured this snapshot
    uint32_t overflowed;    // ... and found a segment longer than its room
    uint32_t totalChunks;
    uint64_t totalBytes;
    uint64_t pad_;
};

// the same three words where the host can read them without a copy (pinned)
struct SnapReport {
    uint64_t totalBytes;
    uint32_t overflowed;
    uint32_t savesMeasured; // written last
};

__host__ __device__ inline uint64_t *snapBytes(SnapHeader *hdr)
{
    return (uint64_t *)(hdr + 1);
}

__host__ __device__ inline uint32_t *snapChunkStart(SnapHeader *hdr, uint32_t num_segments)
{
    return (uint32_t *)(snapBytes(hdr) + num_segments);
}

__host__ __device__ inline SnapSegment *snapSegments(SnapHeader *hdr, uint32_t num_segments)
{
    // (numSegments + 1 dwords of chunk starts, rounded up to 8 bytes)
    return (SnapSegment *)(snapBytes(hdr) + num_segments + (num_segments + 2) / 2);
}

inline size_t snapMetaBytes(uint32_t num_segments)
{
    return sizeof(SnapHeader) + (size_t)num_segments * 8 +
        (size_t)((num_segments + 2) / 2) * 8 + (size_t)num_segments * sizeof(SnapSegment);
}

// inclusive scan of one value per thread over the workgroup; returns the
// thread's inclusive sum, *total the workgroup's
__device__ inline uint64_t snapBlockScan(uint64_t v, uint64_t *lds, uint64_t *total)
{
    const uint32_t tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kSnapThreads; d <<= 1) {
        const uint64_t below = tid >= d ? lds[tid - d] : 0ull;
        __syncthreads();
        lds[tid] += below;
        __syncthreads();
    }
    const uint64_t mine = lds[tid];
    *total = lds[kSnapThreads - 1];
    __syncthreads();
    return mine;
}

// Save, first launch: ONE workgroup.
__global__ void __launch_bounds__(kSnapThreads)
snapshotMeasure(const EcsState *S, SnapHeader *hdr, SnapReport *report)
{
    __shared__ uint64_t lds[kSnapThreads];
    __shared__ uint32_t lds_overflow;
    const uint32_t tid = threadIdx.x;
    const uint32_t num_segments = hdr->numSegments;
    uint64_t *seg_bytes = snapBytes(hdr);
    uint32_t *chunk_start = snapChunkStart(hdr, num_segments);
    const SnapSegment *segments = snapSegments(hdr, num_segments);

    // the ids in use: those of world construction, and the run-time blocks
    // (expandIdStore: world w's k-th block starts at runtimeIdBase +
    // (k * numWorlds + w) * 64) up to the end of the LAST block any world has
    // taken -- not the end of its layer: the store is mapped up to the block a
    // world asked for, so a layer that only low worlds have reached may end
    // past the mapped slots
    uint64_t runtime_end = 0;
    for (int32_t w = (int32_t)tid; w < S->numWorlds; w += (int32_t)kSnapThreads) {
        const int32_t used = S->worldCaches[w].runtimeBlocksUsed;
        if (used > 0) {
            const uint64_t end = (uint64_t)S->runtimeIdBase +
                ((uint64_t)(used - 1) * (uint64_t)S->numWorlds + (uint64_t)w + 1ull) *
                    (uint64_t)kIdsPerBlock;
            runtime_end = end > runtime_end ? end : runtime_end;
        }
    }
    lds[tid] = runtime_end;
    if (tid == 0) lds_overflow = 0u;
    __syncthreads();
    for (uint32_t d = kSnapThreads / 2; d > 0; d >>= 1) {
        if (tid < d && lds[tid + d] > lds[tid]) lds[tid] = lds[tid + d];
        __syncthreads();
    }
    runtime_end = lds[0];
    __syncthreads();
    uint64_t ids_in_use = (uint64_t)(S->numIds > 0 ? S->numIds : 0);
    ids_in_use = runtime_end > ids_in_use ? runtime_end : ids_in_use;

    uint64_t chunks_before = 0, bytes_before = 0;
    for (uint32_t base = 0; base < num_segments; base += kSnapThreads) {
        const uint32_t s = base + tid;
        uint64_t bytes = 0;
        if (s < num_segments) {
            const SnapSegment seg = segments[s];
            uint64_t rows = seg.countArg;
            if (seg.countKind == kSnapTableRows) {
                const int32_t n = S->tables[seg.countArg].numRows;
                rows = (uint64_t)(n > 0 ? n : 0);
            } else if (seg.countKind == kSnapEntities) {
                rows = ids_in_use;
            } else if (seg.countKind == kSnapPersist) {
                rows = S->persistOffset;
            }
            bytes = rows * seg.bytesPerRow;
            if (bytes > seg.roomBytes) {
                // (every column of a table sees the same row count: none of
                // them is copied)
                bytes = 0;
                lds_overflow = 1u;
            }
            seg_bytes[s] = bytes;
        }
        uint64_t total_chunks, total_bytes;
        const uint64_t my_chunks = (bytes + kSnapChunk - 1) / kSnapChunk;
        const uint64_t incl = snapBlockScan(my_chunks, lds, &total_chunks);
        (void)snapBlockScan(bytes, lds, &total_bytes);
        if (s < num_segments) {
            chunk_start[s] = (uint32_t)(chunks_before + incl - my_chunks);
        }
        chunks_before += total_chunks;
        bytes_before += total_bytes;
    }
    __syncthreads();
    if (tid == 0) {
        chunk_start[num_segments] = (uint32_t)chunks_before;
        hdr->totalChunks = (uint32_t)chunks_before;
        hdr->totalBytes = bytes_before;
        hdr->overflowed = lds_overflow;
        hdr->saved = 1u;
        report->totalBytes = bytes_before;
        report->overflowed = lds_overflow;
        __threadfence_system();
        report->savesMeasured = report->savesMeasured + 1u;
    }
}

// Save (second launch) and restore (the only one).  restore: nothing is moved
// unless the snapshot holds a complete save -- and then the executor is told:
// kErrSnapshot in errorFlags (sticky: every later replay's health kernel
// reports it) and in the host's copy of the flags, so that the next
// mwhip_synchronize / mwhip_run fails instead of stepping worlds that were
// not rewound.  (One thread, plain stores: nothing else runs on the stream.)
__global__ void __launch_bounds__(kSnapThreads)
snapshotCopy(EcsState *S, int32_t *stats_host, SnapHeader *hdr, char *data,
             uint32_t restore)
{
    if (restore != 0u && (hdr->saved == 0u || hdr->overflowed != 0u)) {
        if (blockIdx.x == 0u && threadIdx.x == 0u) {
            S->errorFlags = S->errorFlags | kErrSnapshot;
            stats_host[0] = (int32_t)((uint32_t)stats_host[0] | kErrSnapshot);
            __threadfence_system();
        }
        return;
    }
    const uint32_t num_segments = hdr->numSegments;
    const uint64_t *seg_bytes = snapBytes(hdr);
    const uint32_t *chunk_start = snapChunkStart(hdr, num_segments);
    const SnapSegment *segments = snapSegments(hdr, num_segments);
    const uint32_t total = hdr->totalChunks;

    for (uint32_t work = blockIdx.x; work < total; work += gridDim.x) {
        // the last segment that starts at or before this chunk (segments
        // without chunks share their start with the next one: skipped)
        uint32_t lo = 0, hi = num_segments;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (chunk_start[mid] <= work) {
                lo = mid;
            } else {
                hi = mid;
            }
        }
        const SnapSegment seg = segments[lo];
        const uint64_t bytes = seg_bytes[lo];
        const uint64_t off = (uint64_t)(work - chunk_start[lo]) * kSnapChunk;
        if (off >= bytes) continue;     // (cannot happen: chunk_start counts them)
        const uint64_t left = bytes - off;
        const uint32_t n = left < kSnapChunk ? (uint32_t)left : kSnapChunk;

        char *live = seg.liveSlot != nullptr ? (char *)*seg.liveSlot : seg.live;
        char *saved = data + seg.savedOffset;
        if (restore != 0u) {
            copyChunk(live + off, saved + off, n);
        } else {
            copyChunk(saved + off, live + off, n);
        }
    }
}

}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct mwhip_snapshot_rec {
    uint64_t handle = 0;
    std::vector<SnapSegment> segments;
    SnapHeader *metaDev = nullptr;      // header + per-segment arrays
    char *dataDev = nullptr;
    uint64_t dataBytes = 0;
    SnapReport *report = nullptr;       // pinned, device-visible
    SnapReport *reportDev = nullptr;    // ... and its device address
    uint32_t savesQueued = 0;

    ~mwhip_snapshot_rec()
    {
        if (metaDev != nullptr) (void)hipFree(metaDev);
        if (dataDev != nullptr) (void)hipFree(dataDev);
        if (report != nullptr) (void)hipHostFree(report);
    }
};

namespace {

bool isRenderOutput(const mwhip_exec *exec, uint32_t archetype, uint32_t component)
{
    const mwhip_render_layout &lay = exec->renderLayout;
    return exec->haveRenderLayout && archetype == lay.output_archetype &&
        (component == lay.rgb_component || component == lay.depth_component);
}

// The segment table for the memory mapped NOW.  Stream idle.
int layoutSnapshot(mwhip_exec *exec, std::vector<SnapSegment> &out, uint64_t *data_bytes)
{
    const EcsState &hs = exec->hostState;
    const uint32_t W = exec->cfg.num_worlds;
    uint64_t persist_used = 0;
    HIPCHK(hipMemcpy(&persist_used,
        (char *)exec->stateDev + offsetof(EcsState, persistOffset),
        sizeof(persist_used), hipMemcpyDeviceToHost));

    out.clear();
    uint64_t at = 0;
    auto add = [&](void *const *slot, void *live, uint32_t bytes_per_row,
                   uint32_t kind, uint32_t arg, uint64_t room_rows) {
        SnapSegment seg {};
        seg.liveSlot = slot;
        seg.live = (char *)live;
        seg.savedOffset = at;
        seg.roomBytes = room_rows * bytes_per_row;
        seg.bytesPerRow = bytes_per_row;
        seg.countKind = kind;
        seg.countArg = arg;
        if (seg.roomBytes == 0) return;
        out.push_back(seg);
        at += (seg.roomBytes + kSnapAlign - 1) / kSnapAlign * kSnapAlign;
    };
    auto add_fixed = [&](void *live, uint64_t bytes) {
        // (the length is fixed: "rows" of whatever unit divides it)
        const uint32_t unit = bytes % 16 == 0 ? 16u : (bytes % 4 == 0 ? 4u : 1u);
        add(nullptr, live, unit, kSnapFixed, (uint32_t)(bytes / unit), bytes / unit);
    };

    {
        // the service thread maps rows behind the tables under this lock
        std::lock_guard<std::mutex> capacities(exec->growMutex);
        for (uint32_t a = 0; a < exec->archetypes.size(); a++) {
            const ArchetypeRec &arch = exec->archetypes[a];
            if (!arch.registered) continue;
            TableHdr *hdr = hs.tables + a;
            for (uint32_t c = 0; c < arch.numColumns; c++) {
                // the ray caster's outputs are derived state (and by far the
                // largest columns there are): left as they are
                if (isRenderOutput(exec, a, arch.colComponent[c])) continue;
                add(&hdr->columns[c], nullptr, arch.colBytes[c], kSnapTableRows, a,
                    arch.capacity);
            }
            add_fixed(&hdr->numRows, sizeof(int32_t));
            add_fixed(&hdr->needsSort, sizeof(uint32_t));
            static_assert(offsetof(TableHdr, tailRows) ==
                          offsetof(TableHdr, sortedRows) + sizeof(int32_t));
            add_fixed(&hdr->sortedRows, 2 * sizeof(int32_t));
            // (whether the holes of the saved step have all been refilled)
            static_assert(offsetof(TableHdr, plainDestroys) ==
                          offsetof(TableHdr, orderedFreed) + 2 * sizeof(uint32_t));
            add_fixed(&hdr->orderedFreed, 3 * sizeof(uint32_t));
            add_fixed(arch.worldOffsets, (uint64_t)W * sizeof(int32_t));
            add_fixed(arch.worldCounts, (uint64_t)W * sizeof(int32_t));
        }
        add(nullptr, hs.entities, sizeof(EntitySlot), kSnapEntities, 0,
            (uint64_t)hs.entityCapacity);
    }
    add_fixed(hs.worldCaches, (uint64_t)W * sizeof(IdCache));
    add_fixed(hs.worldData, (uint64_t)W * hs.worldDataStride);
    // (a step that allocates from the persistent region moves persistOffset on:
    // room for what is used now and as much again)
    add(nullptr, hs.persistBase, 1, kSnapPersist, 0,
        std::min<uint64_t>(hs.persistCapacity, std::max<uint64_t>(2 * persist_used, 4096)));
    char *state = (char *)exec->stateDev;
    add_fixed(state + offsetof(EcsState, tmpOffset), sizeof(unsigned long long));
    add_fixed(state + offsetof(EcsState, persistOffset), sizeof(unsigned long long));
    add_fixed(state + offsetof(EcsState, idFreeHead), sizeof(unsigned long long));
    add_fixed(state + offsetof(EcsState, numIds), sizeof(int32_t));
    add_fixed(state + offsetof(EcsState, runtimeIdBase), sizeof(int32_t));
    *data_bytes = std::max<uint64_t>(at, kSnapAlign);
    return 0;
}

// (Re)allocates the snapshot for the memory mapped now; what it held is gone.
// A layout that has not changed keeps its buffers.  Stream idle.
int sizeSnapshot(mwhip_exec *exec, mwhip_snapshot_rec &snap)
{
    std::vector<SnapSegment> segments;
    uint64_t data_bytes = 0;
    int rc = layoutSnapshot(exec, segments, &data_bytes);
    if (rc != 0) return rc;
    if (snap.metaDev != nullptr && data_bytes == snap.dataBytes &&
            segments.size() == snap.segments.size() &&
            memcmp(segments.data(), snap.segments.data(),
                   segments.size() * sizeof(SnapSegment)) == 0) {
        return 0;
    }

    if (snap.metaDev != nullptr) (void)hipFree(snap.metaDev);
    if (snap.dataDev != nullptr) (void)hipFree(snap.dataDev);
    snap.metaDev = nullptr;
    snap.dataDev = nullptr;
    snap.dataBytes = 0;
    snap.segments.clear();
    snap.savesQueued = 0;

    const uint32_t n = (uint32_t)segments.size();
    std::vector<char> meta(snapMetaBytes(n), 0);
    SnapHeader *hdr = (SnapHeader *)meta.data();
    hdr->numSegments = n;
    memcpy(snapSegments(hdr, n), segments.data(), n * sizeof(SnapSegment));
    HIPCHK(hipMalloc((void **)&snap.metaDev, meta.size()));
    HIPCHK(hipMemcpy(snap.metaDev, meta.data(), meta.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&snap.dataDev, data_bytes));
    snap.dataBytes = data_bytes;
    snap.segments = std::move(segments);
    memset(snap.report, 0, sizeof(SnapReport));
    return 0;
}

mwhip_snapshot_rec *findSnapshot(mwhip_exec *exec, uint64_t handle)
{
    return findObject(exec != nullptr ? &exec->snapshots : nullptr, handle);
}

uint32_t snapGrid(const mwhip_exec *exec)
{
    return std::max(exec->numCUs, 1u) * 8u;
}

int queueSave(mwhip_exec *exec, mwhip_snapshot_rec &snap)
{
    const EcsState *state = exec->stateDev;
    hipLaunchKernelGGL(snapshotMeasure, dim3(1), dim3(kSnapThreads), 0, exec->stream,
                       state, snap.metaDev, snap.reportDev);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(snapshotCopy, dim3(snapGrid(exec)), dim3(kSnapThreads), 0,
                       exec->stream, exec->stateDev, (int32_t *)nullptr,
                       snap.metaDev, snap.dataDev, 0u);
    HIPCHK(hipGetLastError());
    snap.savesQueued++;
    return 0;
}

// What the host knows of the last save WITHOUT waiting: refuses a restore of a
// snapshot nothing was ever saved into, or whose last save is known to have
// overflowed.  (A save still in flight is judged by the kernel, which moves
// nothing in those two cases.)
int restorable(const mwhip_snapshot_rec &snap)
{
    if (snap.savesQueued == 0) {
        return fail(-3, "snapshot %llu was never saved into",
                    (unsigned long long)snap.handle);
    }
    const uint32_t measured =
        __atomic_load_n(&snap.report->savesMeasured, __ATOMIC_ACQUIRE);
    if (measured == snap.savesQueued && snap.report->overflowed != 0u) {
        return fail(-4, "snapshot %llu: its last save was queued before a table "
                    "grew past the room the snapshot had; save into it again",
                    (unsigned long long)snap.handle);
    }
    return 0;
}

int queueRestore(mwhip_exec *exec, mwhip_snapshot_rec &snap)
{
    int32_t *stats_host = nullptr;
    HIPCHK(hipHostGetDevicePointer((void **)&stats_host, exec->statsHost, 0));
    hipLaunchKernelGGL(snapshotCopy, dim3(snapGrid(exec)), dim3(kSnapThreads), 0,
                       exec->stream, exec->stateDev, stats_host, snap.metaDev,
                       snap.dataDev, 1u);
    HIPCHK(hipGetLastError());
    // Host mirrors after a restore.  Everything the host keeps about the tables
    // is a high-water mark or a choice between kernels that are all correct on
    // any table: capacities only grow (and cover the saved rows: they were
    // mapped when the rows were saved), peakSeen / fillingUntil only throttle
    // the queue, statsHost's rows and peaks are rewritten by the next replay's
    // health kernel and until then at worst ask for growth that the step
    // before the restore justified, bigSort / smallBusy / noCompact / longTails
    // pick the sort path (the one-launch sort, the radix chain and the
    // compaction chain sort any table; the chain starts from the header's
    // sortedRows, which is restored), scrambled is a property of the task
    // graphs, and the grids of the launch graphs stride over the device's row
    // counts (rowsAtGraphBuild only sizes them).  So nothing is reset.
    return 0;
}


int restoreSnapshot(mwhip_exec *exec, uint64_t snapshot, bool wait)
{
    mwhip_snapshot_rec *snap = findSnapshot(exec, snapshot);
    if (snap == nullptr) return unknownObject("snapshot", snapshot);
    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    if (wait) {
        HIPCHK(hipStreamSynchronize(exec->stream));
    }
    int rc = restorable(*snap);
    if (rc != 0) return rc;
    return finishQueued(exec, queueRestore(exec, *snap), wait);
}

}

extern "C" int mwhip_snapshot_create(mwhip_exec *exec, uint64_t *snapshot_out)
{
    carryStale(exec);
    if (exec == nullptr || !exec->stateBuilt || snapshot_out == nullptr) {
        return fail(-2, "snapshot_create: no executor state");
    }
    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    HIPCHK(hipStreamSynchronize(exec->stream));
    // (a snapshot that is not finished frees what it has when it goes)
    std::unique_ptr<mwhip_snapshot_rec> snap(new mwhip_snapshot_rec {});
    HIPCHK(hipHostMalloc((void **)&snap->report, sizeof(SnapReport), hipHostMallocMapped));
    memset(snap->report, 0, sizeof(SnapReport));
    if (hipHostGetDevicePointer((void **)&snap->reportDev, snap->report, 0) != hipSuccess) {
        return fail(-10, "snapshot_create: no device address for pinned memory");
    }
    int rc = sizeSnapshot(exec, *snap);
    if (rc != 0) return rc;
    *snapshot_out = exec->snapshots.insert(std::move(snap));
    return 0;
}

extern "C" void mwhip_snapshot_destroy(mwhip_exec *exec, uint64_t snapshot)
{
    carryStale(exec);
    if (findSnapshot(exec, snapshot) == nullptr) return;
    (void)hipSetDevice(exec->cfg.gpu_id);
    (void)hipStreamSynchronize(exec->stream);
    exec->snapshots.erase(snapshot);
}

extern "C" int mwhip_snapshot_save(mwhip_exec *exec, uint64_t snapshot)
{
    carryStale(exec);
    mwhip_snapshot_rec *snap = findSnapshot(exec, snapshot);
    if (snap == nullptr) return unknownObject("snapshot", snapshot);
    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    // a replay boundary: every row there is lies in mapped memory, and the
    // snapshot gets room for all of that -- no high-water mark to keep
    HIPCHK(hipStreamSynchronize(exec->stream));
    int rc = sizeSnapshot(exec, *snap);
    if (rc != 0) return rc;
    rc = finishQueued(exec, queueSave(exec, *snap), true);
    if (rc != 0) return rc;
    if (snap->report->overflowed != 0u) {
        return fail(-4, "snapshot_save: a segment outgrew the memory mapped for it");
    }
    return 0;
}

// (into the room the snapshot has)
extern "C" int mwhip_snapshot_save_async(mwhip_exec *exec, uint64_t snapshot)
{
    carryStale(exec);
    mwhip_snapshot_rec *snap = findSnapshot(exec, snapshot);
    if (snap == nullptr) return unknownObject("snapshot", snapshot);
    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    return queueSave(exec, *snap);
}

extern "C" int mwhip_snapshot_restore(mwhip_exec *exec, uint64_t snapshot)
{
    carryStale(exec);
    return restoreSnapshot(exec, snapshot, true);
}

extern "C" int mwhip_snapshot_restore_async(mwhip_exec *exec, uint64_t snapshot)
{
    carryStale(exec);
    return restoreSnapshot(exec, snapshot, false);
}

extern "C" uint64_t mwhip_snapshot_bytes(mwhip_exec *exec, uint64_t snapshot)
{
    mwhip_snapshot_rec *snap = findSnapshot(exec, snapshot);
    if (snap == nullptr || snap->savesQueued == 0) return 0;
    (void)hipSetDevice(exec->cfg.gpu_id);
    if (hipStreamSynchronize(exec->stream) != hipSuccess) return 0;
    return snap->report->totalBytes;
}

extern "C" int32_t mwhip_snapshot_segments(mwhip_exec *exec, uint64_t snapshot,
                                           mwhip_snapshot_segment *out, uint32_t max_out)
{
    mwhip_snapshot_rec *snap = findSnapshot(exec, snapshot);
    if (snap == nullptr) return unknownObject("snapshot", snapshot);
    if (snap->savesQueued == 0) return 0;
    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    HIPCHK(hipStreamSynchronize(exec->stream));
    const uint32_t n = (uint32_t)snap->segments.size();
    std::vector<uint64_t> bytes(n);
    HIPCHK(hipMemcpy(bytes.data(), snapBytes(snap->metaDev), n * sizeof(uint64_t),
                     hipMemcpyDeviceToHost));
    std::vector<TableHdr> hdrs(exec->tablesHost.size());
    HIPCHK(hipMemcpy(hdrs.data(), exec->hostState.tables,
                     hdrs.size() * sizeof(TableHdr), hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < n && s < max_out; s++) {
        const SnapSegment &seg = snap->segments[s];
        void *live = seg.live;
        if (seg.liveSlot != nullptr) {
            // (the slot is a field of the device's table headers: the same
            // field of the copy just read)
            const size_t off = (const char *)seg.liveSlot -
                (const char *)exec->hostState.tables;
            memcpy(&live, (const char *)hdrs.data() + off, sizeof(live));
        }
        out[s] = { live, snap->dataDev + seg.savedOffset, bytes[s] };
    }
    return (int32_t)n;
}
