// Host-side internals shared by the translation units of libmadrona_hip.so
// (runtime.hip: the C ABI; runtime_state.hip: device state, world construction,
// table growth; runtime_launch.hip: launch lists and step graphs;
// runtime_kernels.hip: the runtime's own small kernels; output_ring.hip: the
// output rings; snapshot.hip: saving and restoring all world state; digest.hip:
// per-world state digests; world_view.hip: padded per-world views of a table's
// columns; world_write.hip: the same tensors scattered into a table's columns;
// world_reduce.hip: per-world reductions of a table's columns;
// entity_gather.hip: the cells of the entities a run of handles names;
// entity_scatter.hip: cells written into those entities; ray_query.hip: rays
// cast through the worlds' broadphase BVHs by the simulator's kernel;
// box_query.hip: boxes tested through the same BVHs by its second kernel).
// exec_objects.hpp (included in front of mwhip_exec) holds what every executor
// object shares, step_batch.hpp (included at the end) what the step-batched ones
// share; tree_query.hpp, which ray_query.hip and box_query.hip include, what
// those two share.  Not installed.
#pragma once
#include "runtime_internal.hpp"
#include <madrona/tracing.hpp>
#include <cstddef>
#include "render_internal.hpp"

#include <hip/hip_ext.h>

#include <atomic>
#include <chrono>
#include <cinttypes>
#include <cstdarg>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <unordered_map>


// (shared by the translation units, not exported from the library)
#define MWHIP_RT __attribute__((visibility("hidden")))

// ---- errors (runtime.hip) -------------------------------------------------------
MWHIP_RT int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIPCHK(expr) \
    do { \
        hipError_t hipchk_res_ = (expr); \
        if (hipchk_res_ != hipSuccess) { \
            return fail(-10, "%s -> %s (%s:%d)", #expr, \
                hipGetErrorString(hipchk_res_), __FILE__, __LINE__); \
        } \
    } while (0)

MWHIP_RT uint32_t envU32(const char *name, uint32_t fallback);

namespace madrona {
namespace mwhip {

// ---- what the runtime's own kernels share with the host (runtime_kernels.hip) ----
// exclusive scan over a few device arrays (MWHIP_NODE_EXCLUSIVE_SCAN)
constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kScanThreads * kScanItems;

struct ScanState {
    uint32_t ticket;
    uint32_t epoch;
    uint32_t arrivals;
    uint32_t pad;
};

struct ScanNode {
    mwhip_scan_params params;
    ScanState *state;
    unsigned long long *granules;
    uint32_t maxTiles;
};

struct PackArgs {
    const uint32_t *src[MWHIP_PACK_MAX_COLUMNS];
    uint32_t words[MWHIP_PACK_MAX_COLUMNS];     // per row, per column
    uint32_t firstWord[MWHIP_PACK_MAX_COLUMNS]; // of the column inside a record
    uint32_t numColumns;
    uint32_t recordWords;
    uint32_t numRows;
};

// layout of the pinned health record (int32 words)
constexpr uint32_t kStatsRows = 2;                          // [kMaxArchetypes]
constexpr uint32_t kStatsGate = 2 + kMaxArchetypes;         // profiling gate flag
constexpr uint32_t kStatsPeaks = 3 + kMaxArchetypes;        // [kMaxArchetypes]
constexpr uint32_t kStatsReplays = 3 + 2 * kMaxArchetypes;  // replays completed
constexpr uint32_t kStatsTails = 4 + 2 * kMaxArchetypes;    // [kMaxArchetypes]
constexpr uint32_t kStatsWords = 4 + 3 * kMaxArchetypes;

// word of the replay-signal block that counts completed replays of STEP graphs
// only (the ones that start with the input rings); word 0 counts every replay
constexpr uint32_t kStepReplayWord = 16;
// ... and the one that counts completed replays of RENDER graphs (the render
// kind of output rings hangs off it)
constexpr uint32_t kRenderReplayWord = 17;

// host stubs of those kernels (for KernelLaunch::fn / hipLaunchKernel)
MWHIP_RT const void *miscOpsKernelFn();
MWHIP_RT const void *exclusiveScanKernelFn();
MWHIP_RT const void *gateKernelFn();
MWHIP_RT const void *benchWindowMarkerFn();
MWHIP_RT const void *packRowsKernelFn();
MWHIP_RT const void *inputRingKernelFn();
#ifdef MADRONA_TRACING
MWHIP_RT const void *traceMarkKernelFn();
#endif
MWHIP_RT const void *statsKernelFn();

}
}

using namespace madrona;
using namespace madrona::mwhip;

// ---------------------------------------------------------------------------
// executor
// ---------------------------------------------------------------------------
struct ComponentRec {
    bool registered = false;
    uint32_t alignment = 0;
    uint32_t bytes = 0;
};

// Growable device memory: address space reserved up front
// (hipMemAddressReserve), backed 2 MiB at a time (hipMemCreate / hipMemMap), so
// a table can grow without any pointer into it changing -- the reference's GPU
// backend does the same through its host allocator thread (memory.cpp:20-178,
// cuda_exec.cpp:1603-1719).  One handle per 2 MiB chunk: the granule on which
// map + set-access behaved on this ROCm (larger or mixed chunk sizes returned
// hipErrorInvalidValue from hipMemSetAccess).
struct VmRange {
    char *base = nullptr;
    size_t reserved = 0;
    size_t mapped = 0;
    std::vector<hipMemGenericAllocationHandle_t> chunks;
};
static constexpr size_t kVmChunk = (size_t)2 << 20;

struct ArchetypeRec {
    bool registered = false;
    uint32_t id = 0;
    std::vector<uint32_t> comps;        // flattened user components
    uint32_t flags = 0;
    uint32_t maxPerWorld = 0;
    bool singleton = false;
    bool bigSort = false;
    uint32_t smallBusy = 0;     // consecutive reports of a busy one-launch sort           // outgrew the single-launch sort once
    // world sorts of this table take the compaction chain unless something
    // other than world sorts reorders / truncates it (a sort by another key,
    // ClearTmp, a scan node writing its row count: scrambled), or its appended
    // tails keep outgrowing what one workgroup sorts (noCompact)
    bool scrambled = false;
    bool noCompact = false;
    uint32_t longTails = 0;         // steps whose tail exceeded the limit
    int64_t peakSeen = 0;           // largest per-step peak reported so far
    uint32_t fillingUntil = 0;      // replay count until which the queue is kept short
    int32_t singletonOrdinal = -1;
    uint32_t capacity = 0;              // rows backed by memory right now
    uint32_t reservedCapacity = 0;      // rows the address space allows
    uint32_t numColumns = 0;
    uint32_t rowBytes = 0;
    std::vector<void *> primary;
    std::vector<void *> alt;
    // growable archetypes: the ranges behind primary / alt / sort buffers
    std::vector<VmRange *> primaryVm, altVm;
    VmRange *sortVm[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    std::vector<uint32_t> colBytes;
    std::vector<uint32_t> colFlags;
    std::vector<uint32_t> colComponent;
    int32_t *worldOffsets = nullptr;
    int32_t *worldCounts = nullptr;
    // sort scratch (allocated on first use)
    SortState *sortState = nullptr;
    uint32_t *keysA = nullptr, *keysB = nullptr;
    int32_t *idxA = nullptr, *idxB = nullptr;
    unsigned long long *lookback = nullptr;
    int32_t *tileCounts = nullptr;      // compaction chain, per prefix tile
    int32_t *tileTailStart = nullptr;
    int32_t *tailLand = nullptr;        // [capacity] where each sorted tail row lands
    int32_t *moveDest = nullptr;        // [capacity] where each tail row goes (stay mode)
    void **sortColPtrs = nullptr;       // [2 * columns] buffers when a chain started
};

struct QueryRec {
    std::vector<uint32_t> comps;
    uint32_t offset;
    uint32_t numMatching;
    uint32_t flags;
};

struct NodeRec {
    mwhip_node_desc desc;
    std::string name;
    std::vector<int32_t> deps;
    bool carried = false;       // MWHIP_NODE_CARRIED was set in desc.kind
    // MWHIP_NODE_INLINE_GROUP was set in desc.kind: desc.pfor_group_kernel is
    // the group's inlined kernel, desc.component_id the node's place in its
    // member list, desc.archetype_id its declared scratch LDS
    bool inlineGroup = false;
};

struct TaskGraphRec {
    std::vector<NodeRec> nodes;
    std::vector<void *> dataDev;
    std::vector<int32_t> sorted;
    bool built = false;
};

struct LaunchGraph {
    // device memory that belongs to THIS graph (sort batches' site / column /
    // slice tables, scan state, row-snapshot granules ...): released when the
    // graph is rebuilt or freed, not at mwhip_destroy (every rebuild
    // -- growth, a table outgrowing the one-launch sort, set_input_ring -- used
    // to leave the previous graph's buffers allocated)
    std::vector<void *> ownedAllocations;
    std::vector<KernelLaunch> launches;
    std::vector<std::unique_ptr<SortBatch>> sortBatches;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graphExec = nullptr;
    // Launches flagged MWHIP_NODE_CARRIED (KernelLaunch::carried) recompute what
    // the previous replay of this graph left in memory.  A graph that holds some
    // is instantiated a second time without them (the edges are a chain: the
    // neighbours join), and replayGraph picks per replay (carriedReplay,
    // runtime.hip).  MADRONA_MWHIP_CARRY_BROADPHASE=2: with
    // the kernels that check the promise in their place (steadyFn).  Null:
    // nothing to leave out, or this graph may never leave it out (carryAllowed).
    hipGraph_t steadyGraph = nullptr;
    hipGraphExec_t steadyExec = nullptr;
    bool hasCarried = false;
    // decided when the graph is built: no step write in the executor's
    // ReplayExtras, and no exported column of a component the carried launches
    // read (a caller may write an exported column behind the runtime's back)
    bool carryAllowed = false;
    std::string statName;
    std::vector<std::string> statNames;     // backing store for mwhip_kernel_stat::name
    std::vector<uint32_t> taskGraphIds;     // to rebuild after a table grew
    // optional last node: pack exported columns into a send buffer
    bool hasPack = false;
    PackArgs pack {};
    void *packDst = nullptr;
    // the batch ray caster's pass instead of task graphs
    bool isRender = false;

    LaunchGraph() = default;
    LaunchGraph(const LaunchGraph &) = delete;
    LaunchGraph &operator=(const LaunchGraph &) = delete;
    // (a graph that dies on an error path of instantiateLaunchGraph or of a
    // rebuild loop gives back what it had allocated so far; the caller has
    // made sure nothing of it is in flight)
    ~LaunchGraph()
    {
        if (graphExec) (void)hipGraphExecDestroy(graphExec);
        if (graph) (void)hipGraphDestroy(graph);
        if (steadyExec) (void)hipGraphExecDestroy(steadyExec);
        if (steadyGraph) (void)hipGraphDestroy(steadyGraph);
        for (void *p : ownedAllocations) {
            (void)hipFree(p);
        }
    }
};

// Where devAlloc records what it hands out while THIS thread builds a launch
// graph (the graph then owns the memory); another thread's allocations stay with
// their executor.
// (__thread: no dynamic initialisation, so no TLS init function to call from the
// other translation units)
extern MWHIP_RT __thread std::vector<void *> *t_allocScope;   // (runtime_state.hip)

// (needs MWHIP_RT and fail() from above; defines what mwhip_exec holds below)
#include "exec_objects.hpp"
struct mwhip_snapshot_rec;      // (snapshot.hip)
struct mwhip_digest_rec;        // (digest.hip)
struct mwhip_view_rec;          // (world_view.hip)
struct mwhip_write_rec;         // (world_write.hip)
struct mwhip_reduce_rec;        // (world_reduce.hip)
struct mwhip_gather_rec;        // (entity_gather.hip)
struct mwhip_scatter_rec;       // (entity_scatter.hip)
struct mwhip_rays_rec;          // (ray_query.hip)
struct mwhip_boxes_rec;         // (box_query.hip)
struct mwhip_contacts_rec;      // (contact_query.hip)
struct mwhip_shapes_rec;        // (shape_query.hip)

// What a replay carries besides its task graphs.  Every launch graph is built
// from it (the input rings, the step writes and the step scatters open a step graph, the rest are tail stages:
// instantiateLaunchGraph), so it changes only through changeReplayExtras.
struct ReplayExtras {
    // mwhip_set_input_ring
    struct InputRing {
        uint32_t *dst;
        const uint32_t *ring;
        uint32_t slotWords;
        uint32_t numSlots;
        uint32_t firstReplay;   // replays completed when the ring was set
    };
    std::vector<InputRing> inputRings;

    // mwhip_set_output_ring: at most MWHIP_MAX_OUTPUT_RINGS over both kinds
    struct OutputRing {
        const char *src;
        char *ring;
        uint64_t slotBytes;
        uint32_t numSlots;
        uint32_t firstReplay;   // replays of the kind completed when the ring was set
        uint32_t when;          // MWHIP_RING_ON_STEP / MWHIP_RING_ON_RENDER
    };
    std::vector<OutputRing> outputRings;

    // mwhip_set_step_digest: the one every step replay recomputes (0: none)
    uint64_t stepDigest = 0;
    // mwhip_set_step_view: those every step replay recomputes, in one launch
    std::vector<uint64_t> stepViews;
    // mwhip_set_step_write: those every step replay applies, in one launch
    // behind the input rings
    std::vector<uint64_t> stepWrites;
    // mwhip_set_step_reduce: those every step replay recomputes, in one launch
    // behind the step views
    std::vector<uint64_t> stepReduces;
    // mwhip_set_step_gather: those every step replay recomputes, in one launch
    // directly behind the step views (whose slabs they may read)
    std::vector<uint64_t> stepGathers;
    // mwhip_set_step_scatter: those every step replay applies, in three launches
    // directly behind the step writes (no two of them list the same component)
    std::vector<uint64_t> stepScatters;
    // mwhip_set_step_rays: those every step replay recomputes, in one launch
    // behind the step views and in front of the step gathers
    std::vector<uint64_t> stepRays;
    // mwhip_set_step_boxes: those every step replay recomputes, in one launch
    // directly behind the step ray queries
    std::vector<uint64_t> stepBoxes;
    // mwhip_set_step_contacts: those every step replay recomputes, in one
    // launch directly behind the step box queries
    std::vector<uint64_t> stepContacts;
    // mwhip_set_step_shapes: those every step replay recomputes, in one launch
    // directly behind the step contact queries
    std::vector<uint64_t> stepShapes;
};

struct mwhip_exec {
    mwhip_state_config cfg {};
    mwhip_user_entry entry {};
    hipStream_t stream = nullptr;

    std::vector<ComponentRec> components;
    std::vector<ArchetypeRec> archetypes;
    std::unordered_map<uint32_t, std::vector<uint32_t>> bundles;
    std::vector<QueryRec> queries;
    std::vector<uint32_t> queryDataHost;
    uint32_t queryCapacity = 1u << 16;      // reference state.hpp:207
    uint32_t numSingletons = 0;
    bool registrationOpen = false;
    bool stateBuilt = false;

    std::vector<void *> exported;

    EcsState hostState {};
    EcsState *stateDev = nullptr;
    std::vector<TableHdr> tablesHost;
    uint32_t singletonIdEnd = 0;            // rounded up to a block of 64

    void *userCfgDev = nullptr;
    void *worldInitsDev = nullptr;

    std::vector<TaskGraphRec> taskGraphs;
    std::unordered_map<uint64_t, std::unique_ptr<LaunchGraph>> launchGraphs;
    // where devAlloc records what it hands out: the graph being built, or
    // (nullptr) the executor's own list, freed at mwhip_destroy
    uint64_t nextGraphHandle = 1;

    // mwGPU::HostPrint: ring in pinned host memory + the thread that drains it
    // while replays are in flight (replaces the reference's HostPrintCPU
    // thread, src/mw/cuda_exec.cpp)
    // device -> host requests for table memory (mwhip::GrowMailbox) and the
    // lock that orders the service thread against growth between replays
    hipStream_t serviceStream = nullptr;    // fills of freshly mapped memory
    VmRange *entityVm = nullptr;            // entity slots (growable)
    VmRange *tmpVm = nullptr;               // Context::tmpAlloc region (growable)
    GrowMailbox *growMailbox = nullptr;
    std::mutex growMutex;
    bool headersStale = false;      // device headers / graphs lag the mapped rows
    HostPrintRing *printRing = nullptr;
    std::mutex printMutex;
    std::thread printThread;
    std::atomic<bool> printStop { false };
    int32_t *statsHost = nullptr;           // pinned, device-visible
    std::vector<void *> allocations;
    std::vector<std::unique_ptr<VmRange>> vmRanges;
    std::vector<uint32_t> rowsAtGraphBuild; // per archetype, see queryCapacityRows
    uint32_t *replaySignal = nullptr;       // device: replays completed
    uint32_t replaysLaunched = 0;           // host: replays queued
    uint32_t tableGrowth = 1;               // reserved / initial rows
    uint32_t numGrowths = 0;
    bool checkAfterRun = true;
    bool sortCarriesMisc = true;    // MADRONA_MWHIP_SORT_CARRIES_MISC

    ReplayExtras extras;

    // MADRONA_TRACING builds: the device event log (mw_gpu/tracing.hpp), the
    // records of the first steps, the names funcID indexes
    void *deviceTracing = nullptr;
    void *traceCursor = nullptr;
    std::vector<mwGPU::DeviceTracing::DeviceLog> traceLogs;
    std::vector<std::string> traceNames;
    uint32_t traceSteps = 0;
    // MADRONA_MWHIP_SORT_COMPACT: 0 never, 1 world sorts of tables nothing else
    // reorders, 2 every world sort (tests: the chain is correct on any table,
    // its one-workgroup tail sort is just slow when the whole table is "tail")
    uint32_t sortCompaction = 1;
    bool eagerReplay = false;       // MADRONA_MWHIP_EAGER (measurement, replayGraph)
    // ---- carried launches (MWHIP_NODE_CARRIED) ----
    // MADRONA_MWHIP_CARRY_BROADPHASE, read at creation: 0 every replay is full,
    // 1 (default) a replay that directly follows a replay of the same launch
    // graph leaves the carried launches out, 2 every replay is full and the
    // simulator's carried nodes check instead of store (physics.inl)
    uint32_t carryMode = 1;
    // Handle of the launch graph whose replay was the LAST thing this executor
    // was asked to do, 0 if anything else happened since (carryStale): every
    // entry point of mwhip.h except the replay calls, mwhip_synchronize and the
    // pure getters, every rebuild of a launch graph, every failed call.
    uint64_t carryFrom = 0;
    uint64_t carryEpoch = 0;        // g_carryEpoch when carryFrom was set
    std::unordered_map<uint64_t, mwhip_carry_counters> carryCounts;  // by handle
    // component ids the carried nodes read (mwhip_carried_reads) and those of
    // every exported column (mwhip_export_column)
    std::vector<uint32_t> carriedReads;
    // kernel -> the kernel that checks instead of storing (mwhip_carried_check)
    std::unordered_map<const void *, const void *> carriedChecks;
    std::vector<uint32_t> exportedComponents;
    const void *pforGroupKernel = nullptr;  // mwhip_set_pfor_group_kernel
    // mwhip_set_ray_kernel: the simulator's rayQueryKernel (null: it has no
    // broadphase, hence no ray queries)
    const void *rayKernel = nullptr;
    // mwhip_set_box_kernel: the simulator's boxQueryKernel, likewise
    const void *boxKernel = nullptr;
    // mwhip_set_contact_kernel: the simulator's contactQueryKernel (null: it
    // has no rigid-body step, hence no narrowphase) and what it can do
    // (MWHIP_CONTACT_CAP_*)
    const void *contactKernel = nullptr;
    uint32_t contactCaps = 0;
    // mwhip_set_shape_kernel: the simulator's shapeQueryKernel, likewise, the
    // bytes of scratch a wavefront of it needs (a multiple of 256) and the block
    // the first mwhip_shapes_create makes of them (in `allocations`)
    const void *shapeKernel = nullptr;
    uint32_t shapeScratchBytes = 0;
    char *shapeScratch = nullptr;
    uint32_t shapeScratchWaves = 0;
    void *pforBodyScratch = nullptr;        // 8 bytes: where report mode writes
    // MADRONA_MWHIP_EXEC_CONFIG_FILE (the reference's
    // MADRONA_MWGPU_EXEC_CONFIG_FILE, cuda_exec.cpp:2115-2172): per task-graph
    // node (index in execution order) the workgroups per CU its kernel may
    // occupy -- the reference's "blocks per SM" of the megakernel that runs the
    // node --, written by madrona_amd/scripts/profile.py.  0 / absent: default.
    std::vector<uint32_t> nodeWorkgroupsPerCU;
    uint32_t numCUs = 256;

    // batch ray caster: geometry (bottom-level BVHs) + where the ECS keeps what
    // it reads and writes
    bool haveRenderGeometry = false;
    bool haveRenderLayout = false;
    RenderGeometryHost renderGeometry;
    RenderGeometryDev renderGeometryDev {};
    mwhip_render_layout renderLayout {};
    BvhNode *tlasNodes = nullptr;
    PreparedInstance *preparedInstances = nullptr;

    // executor objects by handle (exec_objects.hpp): mwhip_snapshot_create,
    // mwhip_digest_create, mwhip_view_create, mwhip_write_create; what is left goes
    // with the executor
    ExecObjectTable<mwhip_snapshot_rec> snapshots;
    ExecObjectTable<mwhip_digest_rec> digests;
    ExecObjectTable<mwhip_view_rec> views;
    ExecObjectTable<mwhip_write_rec> writes;
    ExecObjectTable<mwhip_reduce_rec> reduces;     // mwhip_reduce_create
    ExecObjectTable<mwhip_gather_rec> gathers;     // mwhip_gather_create
    ExecObjectTable<mwhip_scatter_rec> scatters;   // mwhip_scatter_create
    ExecObjectTable<mwhip_rays_rec> rays;          // mwhip_rays_create
    ExecObjectTable<mwhip_boxes_rec> boxes;        // mwhip_boxes_create
    ExecObjectTable<mwhip_contacts_rec> contacts;  // mwhip_contacts_create
    ExecObjectTable<mwhip_shapes_rec> shapes;      // mwhip_shapes_create
};

// Bumped by what changes device memory or fails without naming an executor
// (mwhip_memcpy_h2d, mwhip_raw_copy_h2d, fail()): every executor of the process
// is stale after it.  (runtime.hip)
extern MWHIP_RT std::atomic<uint64_t> g_carryEpoch;

// The next replay of this executor runs every launch.
inline void carryStale(mwhip_exec *exec)
{
    if (exec != nullptr) exec->carryFrom = 0;
}

// What a steady replay (replayGraph's rule holds) launches for `k`: the launch
// itself, nothing (nullptr: a carried launch, mode 1), or the kernel that checks
// the simulator's promise in its place (mode 2).
inline const void *steadyFn(const mwhip_exec *exec, const KernelLaunch &k)
{
    if (!k.carried) return k.fn;
    if (exec->carryMode == 2u) return k.checkFn != nullptr ? k.checkFn : k.fn;
    return nullptr;
}

// ---- functions one translation unit defines and another calls ----------------------
MWHIP_RT int devAlloc(mwhip_exec *exec, void **out, size_t bytes, bool zero = true);
      // (runtime_state.hip)
MWHIP_RT int vmAlloc(mwhip_exec *exec, void **out, VmRange **range_out,
                   size_t reserve_bytes, size_t map_bytes, bool zero);
      // (runtime_state.hip)
MWHIP_RT void vmFreeAll(mwhip_exec *exec);
      // (runtime_state.hip)
MWHIP_RT int findColumn(const ArchetypeRec &arch, uint32_t component_id);
      // (runtime.hip)
MWHIP_RT int buildDeviceState(mwhip_exec *exec);
      // (runtime_state.hip)
MWHIP_RT void drainHostPrints(mwhip_exec *exec, bool in_flight);
      // (runtime_state.hip)
MWHIP_RT const char *describeError(uint32_t flags);
      // (runtime_state.hip)
MWHIP_RT int launchOne(mwhip_exec *exec, KernelLaunch &k, hipStream_t stream);
      // (runtime_launch.hip)
MWHIP_RT bool compactionEligible(const mwhip_exec *exec, uint32_t archetype_id,
                               uint32_t component_id);
      // (runtime_launch.hip)
MWHIP_RT int sortAllArchetypes(mwhip_exec *exec);
      // (runtime_launch.hip)
MWHIP_RT int constructWorlds(mwhip_exec *exec);
      // (runtime_state.hip)
MWHIP_RT int loadExecConfigFile(mwhip_exec *exec);
      // (runtime_state.hip)
MWHIP_RT void releaseLaunchGraph(LaunchGraph &lg);
      // (runtime_launch.hip)
MWHIP_RT int instantiateLaunchGraph(mwhip_exec *exec,
                                  const std::vector<uint32_t> &ids,
                                  const std::string &stat_name,
                                  std::unique_ptr<LaunchGraph> &out,
                                  const LaunchGraph *pack_from = nullptr);
      // (runtime_launch.hip)
MWHIP_RT void serviceGrowRequests(mwhip_exec *exec);
      // (runtime_state.hip)
MWHIP_RT int growTablesFromDevice(mwhip_exec *exec);
      // (runtime_state.hip)
MWHIP_RT int sortsOutgrown(mwhip_exec *exec);
      // (runtime_state.hip)
MWHIP_RT int growTablesAfterReplay(mwhip_exec *exec);
      // (runtime_state.hip)
MWHIP_RT int collectDeviceTrace(mwhip_exec *exec);
      // (runtime_state.hip)
MWHIP_RT void writeDeviceTrace(mwhip_exec *exec);
      // (runtime_state.hip)
// tail stages of a replay (TailStage, runtime_launch.hip)
MWHIP_RT int stepDigestStage(mwhip_exec *exec, const LaunchGraph &lg,
                             std::vector<KernelLaunch> &out);
      // (digest.hip)
MWHIP_RT int stepViewStage(mwhip_exec *exec, const LaunchGraph &lg,
                           std::vector<KernelLaunch> &out);
      // (world_view.hip)
MWHIP_RT int stepGatherStage(mwhip_exec *exec, const LaunchGraph &lg,
                             std::vector<KernelLaunch> &out);
      // (entity_gather.hip)
MWHIP_RT int checkHandleRequest(mwhip_exec *exec, const char *what,
                                const mwhip_gather_source *source,
                                const uint32_t *component_ids, uint32_t n, const void *out);
      // (entity_gather.hip)
MWHIP_RT int stepRaysStage(mwhip_exec *exec, const LaunchGraph &lg,
                           std::vector<KernelLaunch> &out);
      // (ray_query.hip)
MWHIP_RT int stepBoxesStage(mwhip_exec *exec, const LaunchGraph &lg,
                            std::vector<KernelLaunch> &out);
      // (box_query.hip)
MWHIP_RT int stepContactsStage(mwhip_exec *exec, const LaunchGraph &lg,
                               std::vector<KernelLaunch> &out);
      // (contact_query.hip)
MWHIP_RT int stepShapesStage(mwhip_exec *exec, const LaunchGraph &lg,
                             std::vector<KernelLaunch> &out);
      // (shape_query.hip)
MWHIP_RT int stepScatterStage(mwhip_exec *exec, const LaunchGraph &lg,
                              std::vector<KernelLaunch> &out);
      // (entity_scatter.hip)
MWHIP_RT int stepReduceStage(mwhip_exec *exec, const LaunchGraph &lg,
                             std::vector<KernelLaunch> &out);
      // (world_reduce.hip)
// head stage of a step replay: behind its input rings, in front of its first
// task-graph node (buildLaunchList, runtime_launch.hip)
MWHIP_RT int stepWriteStage(mwhip_exec *exec, const LaunchGraph &lg,
                            std::vector<KernelLaunch> &out);
      // (world_write.hip)
MWHIP_RT int outputRingStage(mwhip_exec *exec, const LaunchGraph &lg,
                             std::vector<KernelLaunch> &out);
      // (output_ring.hip)
MWHIP_RT int rebuildAllLaunchGraphs(mwhip_exec *exec);
      // (runtime.hip)

template <typename T>
inline int devAllocT(mwhip_exec *exec, T **out, size_t count, bool zero = true)
{
    return devAlloc(exec, (void **)out, count * sizeof(T), zero);
}

// The one way exec->extras changes: `change` edits it (non-zero: refused), every
// launch graph is rebuilt from the result, and if either fails the executor
// keeps what it had -- it never claims a ring, digest or view that its graphs do
// not carry, or the reverse.  (Callers return early when there is nothing to
// change: no rebuild.)
template <typename Change>
inline int changeReplayExtras(mwhip_exec *exec, Change &&change)
{
    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    HIPCHK(hipStreamSynchronize(exec->stream));
    const ReplayExtras before = exec->extras;
    int rc = change(exec->extras);
    if (rc == 0) rc = rebuildAllLaunchGraphs(exec);
    if (rc != 0) exec->extras = before;
    return rc;
}

// (needs mwhip_exec, ReplayExtras and changeReplayExtras from above)
#include "step_batch.hpp"
