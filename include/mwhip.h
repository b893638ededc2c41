/* mwhip.h -- C ABI of libmadrona_hip.so, the MI355X (gfx950) many-world ECS
 * task-graph backend.
 *
 * The reference has no FFI for this path: its boundary is the C++ class
 * madrona::MWCudaExecutor (reference include/madrona/mw_gpu.hpp:98-164) plus
 * device code that it JIT-compiles with NVRTC.  This header is the C-ABI that
 * a maintainer would bind instead; madrona_amd/include/madrona/mw_gpu.hpp is a
 * header-only C++ shim over it with the reference's class/method names, so
 * existing simulators compile unchanged.  Every entry point cites the
 * reference interface it replaces.
 *
 * Conventions: plain pointers and sizes only; functions returning int return
 * 0 on success and a negative code on error (the reference aborts through
 * FATAL()/REQ_CUDA(); the C++ shim restores that behaviour by aborting on a
 * non-zero code).  One executor drives one GPU from one host thread.
 */
#ifndef MWHIP_H
#define MWHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MWHIP_ABI_VERSION 9u   /* 9: mwhip_snapshot_*() (all world state saved and restored on the device) and, added under 9 without a bump (no struct a simulator library is compiled against changed), mwhip_set_output_ring() / mwhip_output_ring_recorded() and mwhip_digest_*() / mwhip_set_step_digest() (a per-world hash of chosen columns computed on the device) and mwhip_view_*() / mwhip_set_step_view() (padded per-world tensors of a table's columns) and mwhip_write_*() / mwhip_set_step_write() (padded per-world tensors scattered into a table's columns) and mwhip_reduce_term / mwhip_reduce_*() / mwhip_set_step_reduce() (per-world sums, extrema, counts and alarms of a table's columns) and mwhip_gather_source / mwhip_gather_*() / mwhip_set_step_gather() (the cells of the entities a run of handles in device memory names) and mwhip_scatter_*() / mwhip_set_step_scatter() (cells written into the entities such a run of handles names, the highest index winning among duplicates) and mwhip_rays_desc / mwhip_ray_args / mwhip_set_ray_kernel() / mwhip_rays_*() / mwhip_set_step_rays() (tensors of rays cast through the worlds' broadphase BVHs by a kernel the simulator's code object registers) and mwhip_boxes_desc / mwhip_box_args / mwhip_set_box_kernel() / mwhip_boxes_*() / mwhip_set_step_boxes() (tensors of boxes tested through the same BVHs, the whole list of each box's entities, by a second kernel the simulator's code object registers) and mwhip_contacts_desc / mwhip_contact_args / mwhip_set_contact_kernel() / mwhip_contacts_*() / mwhip_set_step_contacts() (per-world tensors of the touching primitive pairs and their manifolds, the step's narrowphase run from outside by a third kernel the simulator's code object registers) and mwhip_shapes_desc / mwhip_shape_args / mwhip_set_shape_kernel() / mwhip_shapes_*() / mwhip_set_step_shapes() (tensors of posed collision shapes tested against the worlds' bodies, the same narrowphase by a fourth kernel the simulator's code object registers) and MWHIP_NODE_CARRIED / mwhip_broadphase_carry_stats() (launches a steady replay leaves out, a bit of mwhip_node_desc::kind that earlier libraries never set); 8: mwhip_persist_bytes_used() (the persistent region's bump offset); 7: mwhip_node_desc::pfor_group_kernel (a node's body is only called from the group kernel of the code object that defines it); 6: mwhip_node_desc::write_mask (same-dependency nodes whose signatures clash keep their own launches); 5: mwhip_node_desc::pfor_body, mwhip_pfor_body(), mwhip_set_pfor_group_kernel() (side-by-side ParallelFor nodes in one launch); 4: io_declared */

typedef struct mwhip_exec mwhip_exec; /* opaque; == MWCudaExecutor::Impl */

/* == madrona::StateConfig (reference include/madrona/mw_gpu.hpp:25-51), POD,
 * plus the gpu id that MWCudaExecutor::initCUDA(gpu_id) (:104) selected. */
typedef struct mwhip_state_config {
    const void *world_init_ptr;     /* host: num_worlds * num_world_init_bytes */
    uint32_t num_world_init_bytes;
    const void *user_config_ptr;    /* host */
    uint32_t num_user_config_bytes;
    uint32_t num_world_data_bytes;
    uint32_t world_data_alignment;
    uint32_t num_worlds;
    uint32_t num_task_graphs;
    uint32_t num_exported_buffers;
    int32_t gpu_id;
    /* == the parts of madrona::CudaBatchRenderConfig (mw_gpu.hpp:77-96) the
     * render-prep ECS systems need (Optional<CudaBatchRenderConfig> of the
     * MWCudaExecutor constructor, cuda_exec.cpp:2333): side of the square
     * ray-caster outputs (0 = ray caster off), colour + depth or depth only,
     * and one object-space root AABB (6 floats: min xyz, max xyz) per object id
     * for the top-level BVH leaf boxes (host pointer, copied; may be NULL). */
    uint32_t raycast_output_resolution;
    uint32_t raycast_rgbd;
    const float *object_root_aabbs;
    uint32_t num_object_root_aabbs;
    uint32_t pad_;
    /* triangle geometry + materials of the renderable objects (== the
     * geoBVHData / materialData of CudaBatchRenderConfig, which the reference
     * fills from Embree-built MeshBVHs): host memory, copied; the executor
     * builds its own bottom-level BVHs.  NULL: no ray caster. */
    const struct mwhip_render_geometry *render_geometry;
    /* most views a world will ever hold (0: unknown).  Sizes the render-target
     * table: at 64 x 64 RGB-D a row is 32 KiB, and a table of unknown size gets
     * the executor's default rows per world. */
    uint32_t raycast_max_views_per_world;
    uint32_t pad2_;
} mwhip_state_config;

typedef struct mwhip_render_geometry {
    uint32_t num_objects;
    uint32_t num_materials;
    const float *vertices;              /* xyz per vertex, all objects */
    const uint32_t *indices;            /* 3 per triangle, object-local vertex ids */
    const uint32_t *object_vertex_offset;   /* [num_objects + 1] into vertices */
    const uint32_t *object_triangle_offset; /* [num_objects + 1] into indices / 3 */
    const int32_t *object_material;     /* [num_objects] material id of the whole
                                         * mesh (reference MeshBVH::materialIDX,
                                         * mesh_bvh.hpp:304); -1: per triangle
                                         * (triangle_material) or, without those,
                                         * none (white); NULL: -1 everywhere */
    const float *material_color;        /* rgb per material */
    /* ---- per-triangle materials and textures (reference
     * MeshBVH::LeafMaterial / BVHVertex::uv, mesh_bvh.hpp:167-178; Material,
     * :148-156; bvh_raycast.cpp:772-800).  All optional (NULL / 0). ---- */
    const float *vertex_uv;             /* uv per vertex, all objects */
    const int32_t *triangle_material;   /* per triangle, all objects: material id
                                         * or -1 (none: white); read for objects
                                         * whose object_material is -1 */
    const int32_t *material_texture;    /* [num_materials] texture id or -1 */
    uint32_t num_textures;
    uint32_t pad_;
    const struct mwhip_texture *textures;   /* [num_textures] */
} mwhip_render_geometry;

/* An RGBA8 texture, row 0 first (what the reference uploads into a cudaArray of
 * uchar4 and samples through a texture object with wrap addressing, linear
 * filtering and normalised coordinates, render/asset_processor.cpp:312-345). */
typedef struct mwhip_texture {
    uint32_t width;
    uint32_t height;
    const uint8_t *rgba8;               /* width * height * 4 bytes, host memory */
} mwhip_texture;

/* Which tables the batch ray caster reads and writes: set once by
 * RenderingSystem::registerTypes (the type ids are assigned there).
 * Replaces the pointers the reference's render BVH kernels find in their
 * BVHParams (src/mw/device/bvh_raycast.cpp, src/mw/cuda_exec.cpp). */
typedef struct mwhip_render_layout {
    uint32_t renderable_archetype;      /* InstanceData, MortonCode, TLBVHNode */
    uint32_t camera_archetype;          /* PerspectiveCameraData */
    uint32_t light_archetype;           /* LightDesc */
    uint32_t output_archetype;          /* RGBOutputBuffer, DepthOutputBuffer */
    uint32_t instance_component;
    uint32_t morton_component;
    uint32_t tlbvh_component;
    uint32_t camera_component;
    uint32_t light_component;
    uint32_t rgb_component;
    uint32_t depth_component;
    uint32_t pad_;
} mwhip_render_layout;

/* What the simulator's offline-compiled HIP translation unit hands to the
 * executor.  Replaces CompileConfig::userSources + the three entry kernels
 * instantiated by MADRONA_BUILD_MWGPU_ENTRY (reference
 * src/mw/device/include/madrona/mw_gpu_entry.hpp:12-91).  registerTypes and
 * setupTasks run on the HOST here (they only describe types and graph
 * topology); world constructors run on the device. */
typedef struct mwhip_user_entry {
    uint32_t abi_version;
    /* calls WorldT::registerTypes(ECSRegistry&, cfg) -> mwhip_register_* */
    void (*register_types)(mwhip_exec *exec, const void *user_cfg_host);
    /* calls WorldT::setupTasks(TaskGraphManager&, cfg) -> mwhip_tg_add_node */
    void (*setup_tasks)(mwhip_exec *exec, const void *user_cfg_host);
    /* host stub of __global__ void(ecs_state*, const void *cfg_dev,
     *   const void *inits_dev, int32_t num_worlds): placement-new of
     *   WorldT(ctx, cfg, init[w]) for one world per thread
     *   (== entryKernels::initWorlds, mw_gpu_entry.hpp:37-56) */
    const void *init_worlds_kernel;
    /* stores the device ecs_state pointer into the user module's
     * __device__ global (== GPUImplConsts::get().stateManagerAddr) */
    void (*bind_device_state)(void *ecs_state_dev);
} mwhip_user_entry;

/* MWCudaExecutor::MWCudaExecutor(state_cfg, compile_cfg, cu_ctx)
 * (reference src/mw/cuda_exec.cpp:2333-2420): allocates the ECS, runs
 * registerTypes, constructs all worlds on the device, runs setupTasks. */
int mwhip_create(const mwhip_state_config *cfg, const mwhip_user_entry *entry,
                 mwhip_exec **out);
/* MWCudaExecutor::~MWCudaExecutor (cuda_exec.cpp:2484-2530) */
void mwhip_destroy(mwhip_exec *exec);
/* last error text for this thread ("" if none) */
const char *mwhip_last_error(void);

/* ---- ECS registry: StateManager::register* ------------------------------
 * reference src/mw/device/state.cpp:154-378, device state.inl:7-158 */
int mwhip_register_component(mwhip_exec *exec, uint32_t component_id,
                             uint32_t alignment, uint32_t num_bytes);
/* bundle ids carry bit 31 (reference state.hpp:197); nested bundles are
 * flattened in place */
int mwhip_register_bundle(mwhip_exec *exec, uint32_t bundle_id,
                          const uint32_t *component_ids, uint32_t num_components);
/* archetype_flags: the reference's ArchetypeFlags (ecs_flags.hpp) plus, in bit
 * 31, "registered by registerSingleton": exactly one row per world, no head
 * room, never grows. */
#define MWHIP_ARCHETYPE_SINGLETON 0x80000000u
int mwhip_register_archetype(mwhip_exec *exec, uint32_t archetype_id,
                             const uint32_t *component_ids,
                             const uint32_t *component_flags, /* may be NULL */
                             uint32_t num_components, uint32_t archetype_flags,
                             uint32_t max_num_entities_per_world);
/* registerSingleton<T>: archetype with one row per world, entity ids assigned
 * in world order (reference device state.inl:136-151, CPU state.inl:163-179) */
int mwhip_register_singleton(mwhip_exec *exec, uint32_t archetype_id,
                             uint32_t component_id);
/* ECSRegistry::exportColumn (registry.inl:47-51): returns the device address
 * of the column, stable for the executor's lifetime, also stored in `slot` */
void *mwhip_export_column(mwhip_exec *exec, uint32_t archetype_id,
                          uint32_t component_id, int32_t slot);
/* StateManager::makeQuery (device/state.cpp:380-440): appends
 * [archetype, col idx per component]* to the query table; returns its offset */
#define MWHIP_QUERY_ALL_SINGLETON 1u  /* every matched archetype has 1 row/world */
int mwhip_make_query(mwhip_exec *exec, const uint32_t *component_ids,
                     uint32_t num_components, uint32_t *offset_out,
                     uint32_t *num_matching_out, uint32_t *flags_out);
/* Executor-owned device scratch (freed by mwhip_destroy). */
void *mwhip_alloc_device(mwhip_exec *exec, uint64_t num_bytes, int zero);
/* Device memory that outlives any executor (asset tables uploaded before the
 * executor exists: PhysicsLoader, reference src/physics/physics_loader.cpp).
 * gpu_id selects the device; return nullptr / nonzero on failure. */
void *mwhip_raw_alloc(int gpu_id, uint64_t num_bytes);
void mwhip_raw_free(int gpu_id, void *device_ptr);
int mwhip_raw_copy_h2d(int gpu_id, void *dst_device, const void *src_host,
                       uint64_t num_bytes);
int mwhip_raw_copy_d2h(int gpu_id, void *dst_host, const void *src_device,
                       uint64_t num_bytes);
/* Small table of module-private device pointers inside ecs_state
 * (ecs_state::moduleData[slot], slot < 4); e.g. the physics module's scratch. */
int mwhip_set_module_data(mwhip_exec *exec, uint32_t slot, void *device_ptr);
void *mwhip_get_module_data(mwhip_exec *exec, uint32_t slot);
/* rows every column of the archetype's table can ever hold (the address space
 * reserved for it; memory is mapped behind it as the table grows) */
uint32_t mwhip_archetype_capacity(mwhip_exec *exec, uint32_t archetype_id);
/* how many times a table has been grown so far (tests / monitoring) */
uint32_t mwhip_num_table_growths(mwhip_exec *exec);
/* Cumulative counters of one table's sort node (device-resident, read after
 * waiting for the executor's stream; tests / monitoring).  A compaction run
 * that moves no surviving row of the sorted prefix patches the few new rows in
 * place ("stay mode", MADRONA_MWHIP_SORT_STAY=0 turns it off) instead of
 * gathering every column into its twin: stay_runs counts those runs, and
 * rows_copied the rows the chains' gather kernel copied per column (the moved
 * rows of a stay run, every row of the sorted table otherwise). */
typedef struct mwhip_sort_counters {
    uint64_t runs;          /* chain or single-launch runs that sorted */
    uint64_t stay_runs;
    uint64_t rows_copied;
    uint64_t rows_in;       /* rows the sorted tables held before / after */
    uint64_t rows_out;
    uint64_t tail_rows;     /* compaction chain: rows behind the sorted prefix */
} mwhip_sort_counters;
/* 0: *out filled; 1: the table has never been part of a sort node (*out
 * zeroed); -1: no such archetype id (ids are dense below the first -1);
 * -2: the device could not be read */
int mwhip_sort_stats(mwhip_exec *exec, uint32_t archetype_id,
                     mwhip_sort_counters *out);
/* Row reuse (Context::destroyEntityOrdered / makeEntityOrdered with
 * OrderedRows::Reuse; MADRONA_MWHIP_ROW_REUSE=0 turns it off): rows created in
 * the slot a destroy of the same invocation freed, and world sorts of the table
 * that found every hole refilled that way and did nothing (they are not counted
 * in mwhip_sort_counters::runs).  Same return values as mwhip_sort_stats. */
typedef struct mwhip_sort_reuse_counters {
    uint64_t skipped_runs;
    uint64_t rows_reused;
} mwhip_sort_reuse_counters;
int mwhip_sort_reuse_stats(mwhip_exec *exec, uint32_t archetype_id,
                           mwhip_sort_reuse_counters *out);
/* the persistent region's current bump offset in bytes (device rawAlloc /
 * HostAllocator: mwhip::persistAlloc, 16-B granules): right after creation,
 * what the last constructor pass took; device code that allocates there while
 * steps run moves it on.  Read only (tests / monitoring).  ~0ull on error. */
uint64_t mwhip_persist_bytes_used(mwhip_exec *exec);
/* device address of the archetype's table header (mwhip::TableHdr) */
void *mwhip_table_header(mwhip_exec *exec, uint32_t archetype_id);
/* copies `count` words of the query table starting at `offset` */
int mwhip_get_query_data(mwhip_exec *exec, uint32_t offset, uint32_t count,
                         uint32_t *out);
/* address of the device-resident ecs_state (valid after mwhip_create's
 * register phase) and of per-world user data */
void *mwhip_device_state(mwhip_exec *exec);
void *mwhip_world_data(mwhip_exec *exec, uint32_t world_idx);
uint32_t mwhip_num_worlds(const mwhip_exec *exec);
/* the ray caster's output resolution / RGBD flag the executor was created with
 * (registerTypes sizes the render-target components from them,
 * reference src/render/ecs_system.cpp:385-404) */
void mwhip_render_config(const mwhip_exec *exec, uint32_t *resolution_out,
                         uint32_t *rgbd_out);
uint32_t mwhip_render_max_views(const mwhip_exec *exec);
/* Host-side preview of what mwhip_create builds from a geometry description (no
 * GPU needed): per object the number of bottom-level BVH nodes, whether the mesh
 * is its own axis-aligned bounds seen from outside (such objects are intersected
 * as slabs + the two triangles of the entry face), and the object-space bounds
 * (6 floats each).  Any output may be NULL.  Returns 0, or -1 with
 * mwhip_last_error() set when the description is malformed. */
int mwhip_render_geometry_info(const struct mwhip_render_geometry *geometry,
                               uint32_t *num_nodes_out, uint32_t *is_box_out,
                               float *bounds_out);
int mwhip_set_render_layout(mwhip_exec *exec, const mwhip_render_layout *layout);
/* MWCudaExecutor::buildRenderGraph (reference mw_gpu.hpp:140, cuda_exec.cpp:
 * 2294-2331): a launch graph that builds every world's top-level BVH over its
 * (Morton-sorted) instances and ray-casts every view into the render-target
 * columns.  Run it after the step graph (mwhip_run / mwhip_run_async). */
int mwhip_build_render_graph(mwhip_exec *exec, uint64_t *graph_out);
uint32_t mwhip_num_task_graphs(const mwhip_exec *exec);

/* ---- task graph: TaskGraph::Builder -------------------------------------
 * reference src/mw/device/taskgraph_utils.cpp:30-146 + taskgraph.inl:59-111 */
enum mwhip_node_kind {
    MWHIP_NODE_KERNEL = 0,        /* user/system kernel: ParallelFor, custom node */
    MWHIP_NODE_SORT_ARCHETYPE = 1,/* SortArchetypeNode<A,C> (sort_archetype.cpp) */
    MWHIP_NODE_CLEAR_TMP = 2,     /* ClearTmpNode<A> (taskgraph_utils.cpp:171-190) */
    MWHIP_NODE_RESET_TMP_ALLOC = 3,/* ResetTmpAllocNode (:216-230) */
    MWHIP_NODE_RECYCLE = 4,       /* RecycleEntitiesNode (:192-214); no-op here */
    /* In-place exclusive prefix sum over up to 8 device arrays treated as one
     * sequence (node_data = mwhip_scan_params).  Building block of the
     * deterministic "count -> scan -> fill" emission of temporaries that
     * replaces arrival-order atomics. */
    MWHIP_NODE_EXCLUSIVE_SCAN = 5
};
/* OR-ed into mwhip_node_desc::kind (added under ABI 9: libraries built before it
 * never set the bit): the node's launches recompute what is already in memory
 * when nothing but replays of the same launch graph happened since the previous
 * replay -- the simulator's promise, e.g.
 * PhysicsSystem::setupBroadphaseTasks(..., BroadphaseInputs::CarriedOver).  A
 * launch graph that holds such launches is instantiated with and without them,
 * and a replay that directly follows a replay of the same graph runs the one
 * without (DESIGN.md section 30 has the whole rule; MADRONA_MWHIP_CARRY_BROADPHASE
 * = 0: never).  Building a launch graph fails when a task graph of it has a
 * flagged node that no unflagged node of the same name follows in the task
 * graph's order: there would be nothing to carry over. */
#define MWHIP_NODE_CARRIED 0x80000000u
/* OR-ed into mwhip_node_desc::kind of a ParallelFor node (added under ABI 9 like
 * the bit above): the simulator named the node as member of a group at compile
 * time (madrona::SideBySide, taskgraph.hpp).  Such a node is a node like any
 * other -- its own kernel, its pfor_body -- and, where it says otherwise today,
 * three fields say more:
 *   pfor_group_kernel  the group's INLINED kernel, __global__ void(ecs_state *,
 *                      const mwhip_pfor_inline_group *), which calls every
 *                      member's body directly; the node's pointer group kernel is
 *                      the executor's (mwhip_set_pfor_group_kernel)
 *   component_id       the node's index in that kernel's member list
 *   archetype_id       bytes of static LDS the node's system uses as scratch
 *                      (madrona::mwhip::systemScratchLDS; 0: none).  A node whose
 *                      own kernel carries exactly that much static LDS carries
 *                      no row-appender marker on top of it: it cannot append
 *                      rows
 * Consecutive launches that name the same inlined kernel and pass every
 * condition of a grouped launch (same dependencies, no carried member, no member
 * that can append rows, no write clash, same task graph) become ONE launch of
 * it, whatever registers their own kernels take (DESIGN.md section 34;
 * MADRONA_MWHIP_GROUP_INLINE=0: never).  Every other member is treated as if the
 * bit were not set. */
#define MWHIP_NODE_INLINE_GROUP 0x40000000u

#define MWHIP_SCAN_MAX_SEGMENTS 8
typedef struct mwhip_scan_params {
    uint32_t num_segments;
    uint32_t capacity;              /* total_out is clamped to this; overflow raises
                                     * the table-overflow device error */
    uint32_t *data[MWHIP_SCAN_MAX_SEGMENTS];         /* device, scanned in place */
    const int32_t *lengths[MWHIP_SCAN_MAX_SEGMENTS]; /* device-resident lengths */
    int32_t *total_out;             /* device; e.g. a table's row count */
    uint32_t *needs_sort_out;       /* optional device flag set to 1 if total > 0 */
} mwhip_scan_params;

enum mwhip_count_mode {
    MWHIP_COUNT_QUERY_ROWS = 0,   /* one invocation per row of the query's tables */
    MWHIP_COUNT_FIXED = 1,        /* fixed_count invocations */
    MWHIP_COUNT_PER_WORLD = 2     /* one invocation per world */
};

/* Query resolution passed BY VALUE in the kernel-argument segment of
 * ParallelFor kernels: the matched tables' header addresses and the column
 * index of every component, so a kernel starts with one round trip (row count +
 * column pointers) instead of walking ecs_state -> query table -> table.
 * Queries matching more archetypes / components than fit set num_inline = 0
 * and the kernel walks the query table (mwhip_make_query) instead. */
#define MWHIP_PFOR_MAX_INLINE 4
#define MWHIP_PFOR_MAX_COMPONENTS 24
typedef struct mwhip_pfor_args {
    uint32_t num_matching;
    uint32_t num_inline;
    void *tables[MWHIP_PFOR_MAX_INLINE];            /* device table headers */
    uint16_t columns[MWHIP_PFOR_MAX_INLINE][MWHIP_PFOR_MAX_COMPONENTS];
    /* Non-NULL for nodes whose system can append rows (makeEntity /
     * makeTemporary reachable from the kernel): per-node device state through
     * which the first workgroup to arrive fixes the row count of every matched
     * table for the whole launch -- the reference evaluates numInvocations
     * once per node (device taskgraph.inl:164-188), so rows created during a
     * node are never visited by it.  The kernel is then launched with
     * 4 * num_matching bytes of dynamic LDS. */
    void *row_sync;
} mwhip_pfor_args;

typedef struct mwhip_node_desc {
    uint32_t kind;
    const char *name;             /* for profiles; copied */
    /* MWHIP_NODE_KERNEL: host stub of
     *   __global__ void(ecs_state*, void *node_data_dev, uint32_t a0, uint32_t a1)
     * or, when wants_pfor_args != 0 (count_mode MWHIP_COUNT_QUERY_ROWS),
     *   __global__ void(ecs_state*, void *node_data_dev, uint32_t a0, uint32_t a1,
     *                   mwhip_pfor_args query) */
    const void *kernel;
    uint32_t wants_pfor_args;
    int32_t node_data_id;         /* from mwhip_tg_add_node_data, or -1 */
    uint32_t arg0, arg1;
    uint32_t count_mode;
    uint32_t fixed_count;
    uint32_t threads_per_invocation;
    uint32_t query_offset;        /* MWHIP_COUNT_QUERY_ROWS */
    uint32_t num_matching;
    uint32_t bytes_per_row;       /* algorithmic bytes for rooflines */
    /* SORT / CLEAR_TMP */
    uint32_t archetype_id;
    uint32_t component_id;
    /* bytes_per_row comes from a read / write set declared next to the system
     * (1; madrona::mwhip::systemIO, taskgraph.inl) or from the signature rule
     * (0: const T & = read, T & = read + write -- an upper bound).  SURVEY §8d;
     * the reference's per-row contract is device taskgraph.inl:164-300. */
    uint32_t io_declared;
    /* ParallelFor nodes (items_per_invocation == 1): device address of the
     * node's body as a __device__ function (mwhip_pfor_body), or NULL.  Nodes
     * that name the SAME dependencies, cannot append rows and carry a body are
     * run side by side in ONE launch of the simulator's group kernel
     * (mwhip_set_pfor_group_kernel): blockIdx.y selects the node.  The reference
     * runs independent nodes of its task graph one after the other
     * (device taskgraph.cpp:142-317); results are the same by the independence
     * the simulator declared with its dependency lists. */
    const void *pfor_body;
    /* ParallelFor nodes: bit i set = the system may write component i of its
     * query (in query order): a non-const reference in its signature.  The
     * runtime does not put two nodes into one launch when one of them writes a
     * component the other one names on a table both match (the reference runs
     * them one after the other, device taskgraph.cpp:142-317: same-dependency
     * siblings may still rely on registration order).  0 with pfor_body set
     * means "writes nothing"; nodes built without a signature pass ~0u. */
    uint32_t write_mask;
    /* ParallelFor nodes with a pfor_body: the group kernel of the code object
     * that defines the body (its registers, scratch and LDS were sized with this
     * body in it).  Only nodes that name the SAME group kernel share a launch,
     * and that kernel is the one launched.  NULL: the executor's default,
     * mwhip_set_pfor_group_kernel(). */
    const void *pfor_group_kernel;
} mwhip_node_desc;

/* Members of a grouped launch, in device memory (the group kernel's argument). */
#define MWHIP_PFOR_GROUP_MAX 6
typedef struct mwhip_pfor_group {
    uint32_t count;
    uint32_t pad_;
    const void *body[MWHIP_PFOR_GROUP_MAX];        /* void (*)(ecs_state *, uint32_t,
                                                     * uint32_t, const mwhip_pfor_args *) */
    uint32_t query_offset[MWHIP_PFOR_GROUP_MAX];
    uint32_t num_matching_and_flags[MWHIP_PFOR_GROUP_MAX];
    mwhip_pfor_args query[MWHIP_PFOR_GROUP_MAX];
} mwhip_pfor_group;

/* Members of an inlined grouped launch (MWHIP_NODE_INLINE_GROUP), in device
 * memory, indexed by the member's place in the kernel's list.  The grid is
 * one-dimensional: member i runs in workgroups [first_workgroup[i],
 * first_workgroup[i] + num_workgroups[i]) of 256 threads, the workgroups a
 * launch of its own would have had; num_workgroups[i] == 0: not in this launch. */
typedef struct mwhip_pfor_inline_group {
    uint32_t first_workgroup[MWHIP_PFOR_GROUP_MAX];
    uint32_t num_workgroups[MWHIP_PFOR_GROUP_MAX];
    uint32_t query_offset[MWHIP_PFOR_GROUP_MAX];
    uint32_t num_matching_and_flags[MWHIP_PFOR_GROUP_MAX];
    mwhip_pfor_args query[MWHIP_PFOR_GROUP_MAX];
} mwhip_pfor_inline_group;

/* (the reference's TaskGraph::maxNodeDataBytes is 256; larger here because a
 * node's data is what its kernel reaches with one load from its arguments) */
#define MWHIP_MAX_NODE_DATA_BYTES 2048u

/* TaskGraph::Builder::constructNodeData (taskgraph.inl:43-57): copies a node
 * data block (<= MWHIP_MAX_NODE_DATA_BYTES) to the device; several nodes may
 * share one block.
 * Returns the data id >= 0 or a negative error. */
int32_t mwhip_tg_add_node_data(mwhip_exec *exec, uint32_t taskgraph_id,
                               const void *data, uint32_t num_bytes);
/* device address of a node data block (TaskGraph::getNodeData) */
void *mwhip_tg_node_data(mwhip_exec *exec, uint32_t taskgraph_id, int32_t data_id);
/* TaskGraph::Builder::registerNode (taskgraph_utils.cpp:30-72).  Nodes are
 * ordered with the reference's own "first unqueued node whose dependencies
 * are queued" rule (taskgraph_utils.cpp:74-146).  Returns node id >= 0. */
int32_t mwhip_tg_add_node(mwhip_exec *exec, uint32_t taskgraph_id,
                          const mwhip_node_desc *desc, const int32_t *deps,
                          uint32_t num_deps);

/* Device address of a ParallelFor kernel's body: launches `kernel` (host stub of
 * a parallelForKernel instantiation) once in its report mode
 * (num_matching_and_flags = 0xFFFFFFFF: thread 0 stores the address of the
 * instantiation's __device__ body at node_data_dev and returns).  NULL on
 * error. */
const void *mwhip_pfor_body(mwhip_exec *exec, const void *kernel);
/* The simulator's group kernel -- __global__ void(ecs_state *, const
 * mwhip_pfor_group *), in the SAME code object as the bodies (device function
 * addresses are only called from the module that defines them). */
int mwhip_set_pfor_group_kernel(mwhip_exec *exec, const void *kernel);

/* compute units of the executor's device (kernel nodes that size a persistent
 * grid themselves) */
uint32_t mwhip_device_cus(const mwhip_exec *exec);

/* ---- execution ----------------------------------------------------------*/
/* MWCudaExecutor::buildLaunchGraph(Span<const uint32_t>, stat_name)
 * (cuda_exec.cpp:2174-2292): captures one hipGraph running the given task
 * graphs back to back.  graph_out is a handle owned by the executor. */
int mwhip_build_launch_graph(mwhip_exec *exec, const uint32_t *taskgraph_ids,
                             uint32_t num_taskgraphs, const char *stat_name,
                             uint64_t *graph_out);
void mwhip_free_launch_graph(mwhip_exec *exec, uint64_t graph);
/* MWCudaExecutor::run (cuda_exec.cpp:2756-2794): synchronous */
int mwhip_run(mwhip_exec *exec, uint64_t graph);
/* MWCudaExecutor::runAsync (:2796-2800).  Replays of ONE executor's launch
 * graphs run one at a time, in the order they were queued -- queue them on one
 * stream (the executor's own, mwhip_stream, or one of the caller's): nodes that
 * can append rows agree on their row counts through a per-replay tag, and two
 * graphs of one executor in flight at once on different streams would not
 * (they time out with a device error, they do not hang). */
int mwhip_run_async(mwhip_exec *exec, uint64_t graph, void *hip_stream);
/* the executor's private stream (cu::makeStream, cuda_exec.cpp:2342) */
void *mwhip_stream(mwhip_exec *exec);
/* Waits for everything queued on the executor's private stream (replays started
 * with mwhip_run_async on mwhip_stream()) and returns the health of the last
 * replay like mwhip_run does (new: the reference leaves this to the caller's
 * cudaStreamSynchronize). */
int mwhip_synchronize(mwhip_exec *exec);
/* What the MWHIP_NODE_CARRIED nodes of this executor read: component ids, any
 * archetype (the sets of several calls add up).  While a column of one of them
 * is exported (mwhip_export_column) every replay runs the carried launches: a
 * caller may write an exported column without the runtime seeing it.  Called
 * by whoever adds the flagged nodes (PhysicsSystem::setupBroadphaseTasks). */
int mwhip_carried_reads(mwhip_exec *exec, const uint32_t *component_ids,
                        uint32_t num_components);
/* MADRONA_MWHIP_CARRY_BROADPHASE=2: every replay that would have left out a
 * MWHIP_NODE_CARRIED launch of `kernel` runs `check_kernel` (same signature,
 * same grid) in its place: it compares what `kernel` would store with what is
 * stored, raises a device error flag on a difference and stores nothing -- how
 * a simulator author finds a broken promise.  A carried kernel without one is
 * simply run. */
int mwhip_carried_check(mwhip_exec *exec, const void *kernel,
                        const void *check_kernel);
/* Replays of launch graph `graph` that ran without its MWHIP_NODE_CARRIED
 * launches, and replays that ran all of them (every replay of a graph that has
 * no such launch is a full one).  Counted when a replay is queued; a rebuild of
 * the graph (growth, rings, step digests ...) keeps the counts.  Pure getter.
 * Non-zero for an unknown handle. */
typedef struct mwhip_carry_counters {
    uint64_t carried_replays;
    uint64_t full_replays;
} mwhip_carry_counters;
int mwhip_broadphase_carry_stats(mwhip_exec *exec, uint64_t graph,
                                 mwhip_carry_counters *out);
/* MWCudaExecutor::getExported (cuda_exec.cpp:2802-2805) */
void *mwhip_get_exported(const mwhip_exec *exec, uint32_t slot);

/* ---- introspection for parity dumps / measurement (new) ----------------- */
int32_t mwhip_num_rows(mwhip_exec *exec, uint32_t archetype_id);
/* Copies column `component_id` of `archetype_id`, rows grouped by world in
 * world order (== concatenating the reference CPU backend's per-world
 * tables, state.inl:368-377); world_counts[num_worlds] receives rows/world.
 * Returns total rows, -1 on error, -2 if dst is too small. */
int64_t mwhip_dump_column(mwhip_exec *exec, uint32_t archetype_id,
                          uint32_t component_id, void *dst, uint64_t dst_bytes,
                          int32_t *world_counts);
/* The same column in TABLE order: every row below the table's row count
 * (destroyed rows included), no grouping by world.  Returns rows, -1 on error,
 * -2 if dst is too small. */
int64_t mwhip_dump_column_raw(mwhip_exec *exec, uint32_t archetype_id,
                              uint32_t component_id, void *dst,
                              uint64_t dst_bytes);
int mwhip_memcpy_d2h(void *dst_host, const void *src_dev, uint64_t num_bytes);
int mwhip_memcpy_h2d(void *dst_dev, const void *src_host, uint64_t num_bytes);
/* to host memory from wherever `src` lives (host or device: a renderer's asset
 * buffers, reference render/cuda_batch_render_assets.hpp, may be either) */
int mwhip_memcpy_any(void *dst_host, const void *src, uint64_t num_bytes);

/* Packs `num_columns` exported columns into one row-major record per row:
 * dst[row] = column 0's words | column 1's words | ...  (4-byte words;
 * words_per_row[c] of them from src_columns[c] + row * words_per_row[c]).  Queued
 * on the executor's stream, i.e. ordered after the replays queued before it --
 * the send buffer of the one observation all-gather per step of a multi-GPU run
 * (the reference hands the column itself to ncclAllGather).
 * Pointers are device pointers; the descriptor arrays are read before the call
 * returns. */
#define MWHIP_PACK_MAX_COLUMNS 16
/* The same packing as the LAST node of a copy of launch graph `base_graph`
 * (a foreign kernel between two replays costs ~35 us of lost launch
 * pipelining on this runtime; inside the graph it costs its own ~4 us).
 * Callers that overlap the collective with the next replay build two such
 * graphs, one per send buffer, and alternate. */
int mwhip_build_launch_graph_with_pack(mwhip_exec *exec, uint64_t base_graph,
                                       uint32_t num_columns,
                                       const void *const *src_columns,
                                       const uint32_t *words_per_row,
                                       uint32_t num_rows, void *dst,
                                       uint64_t *graph_out);
/* Makes `hip_stream` wait for every replay queued so far (mwhip_run_async on
 * the executor's stream) without putting anything on the executor's stream: the
 * last kernel of each replay bumps a counter in signal memory that the waiting
 * stream polls (hipStreamWaitValue32). */
int mwhip_stream_wait_replays(mwhip_exec *exec, void *hip_stream);
int mwhip_pack_rows(mwhip_exec *exec, uint32_t num_columns,
                    const void *const *src_columns,
                    const uint32_t *words_per_row, uint32_t num_rows,
                    void *dst);

/* Device-resident input ring: the k-th replay of a step graph of this executor
 * (any graph from mwhip_build_launch_graph; replays of the render graph neither
 * read nor advance the rings; k = 0, 1, ...) after this call starts by copying slot k % num_slots
 * of `ring` (num_slots x slot_bytes, device memory, whole dwords) into `dst` -- normally an exported
 * action column (mwhip_exported) --, so that a policy's outputs for the next
 * steps can be queued with the replays that consume them; nothing foreign sits
 * on the executor's stream between two graph launches (which costs 20-35 us of
 * launch pipelining each).  ring == NULL removes the ring of
 * `dst`.  The ring belongs to the caller and must stay allocated until it is
 * removed or the executor destroyed.  Rebuilds the launch graphs (handles stay
 * valid); waits for the executor's stream.  (No reference counterpart: its managers write the action
 * tensor between steps, include/madrona/mw_gpu.hpp:146 runAsync + PyTorch.) */
int mwhip_set_input_ring(mwhip_exec *exec, void *dst, const void *ring,
                         uint64_t slot_bytes, uint32_t num_slots);

/* Device-resident output rings (added under ABI 9): the k-th replay after this
 * call (k = 0, 1, ...) of ANY graph of the executor of kind `when` -- step graphs
 * (mwhip_build_launch_graph, mwhip_build_launch_graph_with_pack) or render
 * graphs (mwhip_build_render_graph) -- copies slot_bytes bytes from `src` --
 * normally an exported column, any device address works -- into
 * ring + (k % num_slots) * slot_bytes, as its last act before its health kernel
 * (behind the pack node of a graph that has one).  K queued replays so leave a
 * time-major [K, ...] trajectory behind with nothing foreign on the executor's
 * stream between two graph launches.  Step replays do not
 * advance render rings nor render replays step rings; inside one step replay
 * the input rings and the output rings see the same k: slot k holds what the
 * step that consumed action slot k produced.  slot_bytes is any count >= 1
 * (images, 1-byte flags): the copy is 16 bytes, 4 bytes or 1 byte wide by the
 * alignment of source and slot, chosen per replay on the device.  All rings of
 * one kind share ONE kernel launch per replay.
 * ring == NULL removes the ring of (src, when); setting a pair that has a ring
 * replaces it and restarts k at 0.  At most MWHIP_MAX_OUTPUT_RINGS rings per
 * executor over both kinds.  The ring is the caller's memory: it must stay
 * allocated until it is removed or the executor destroyed, and not reading a
 * slot while a queued replay rewrites it is the caller's job.  Like
 * mwhip_set_input_ring: waits for the executor's stream and rebuilds the launch
 * graphs (handles stay valid).  The rings keep their position over later
 * rebuilds (table growth, mwhip_set_input_ring); a snapshot restore does not
 * rewind them (they hang off the replay counters).
 * Errors (non-zero, text in mwhip_last_error(), nothing changed): a null src;
 * zero slots or zero bytes with a non-null ring; a seventeenth ring; an unknown
 * `when`.  (No reference counterpart; its per-step recorder,
 * madrona::viz::Recorder, is render side only.) */
#define MWHIP_MAX_OUTPUT_RINGS 16
#define MWHIP_RING_ON_STEP   0u   /* recorded by every replay of a step graph   */
#define MWHIP_RING_ON_RENDER 1u   /* recorded by every replay of a render graph */
int mwhip_set_output_ring(mwhip_exec *exec, const void *src, void *ring,
                          uint64_t slot_bytes, uint32_t num_slots, uint32_t when);
/* Waits for the executor's stream; *replays_out = replays that have recorded
 * into the ring of (src, when) since it was set (NOT modulo num_slots).
 * The device counts replays in 32 bits: the count returns to 0 after 2^32
 * replays of that kind since the ring was set, and at that point the slot
 * position jumps unless num_slots is a power of two (set the ring again
 * before then; mwhip_set_input_ring's rings share this).
 * Non-zero (and a message) when the pair has no ring. */
int mwhip_output_ring_recorded(mwhip_exec *exec, const void *src, uint32_t when,
                               uint64_t *replays_out);

/* Queues a one-wave marker kernel (benchWindowMarker) on the executor's stream:
 * a pair of them brackets a measurement window in a rocprofv3 kernel trace
 * (profiles/summarize_rocprof.py trims to it).  Measurement only. */
int mwhip_mark_window(mwhip_exec *exec, uint32_t id);

/* Per-kernel timing with HIP events on the executor's stream (replaces the
 * reference's device tracing, mw_gpu/tracing.hpp).  Runs the launch graph's
 * kernels eagerly `reps` times with an event pair around every kernel. */
typedef struct mwhip_kernel_stat {
    const char *name;       /* node name + kernel role, owned by the executor */
    uint32_t node_kind;
    uint32_t archetype_id;
    double avg_us;          /* mean duration of this kernel per step */
    double algo_bytes;      /* mean algorithmic bytes per launch */
    double rows;            /* mean rows / invocations processed per launch */
    uint32_t io_declared;   /* algo_bytes from a declared read / write set (1),
                             * from the signature rule (0) */
    uint32_t workgroups;    /* grid of the launch */
    uint32_t node_index;    /* position of the node in its task graph's execution
                             * order (the key of MADRONA_MWHIP_EXEC_CONFIG_FILE),
                             * 0xFFFFFFFF for kernels that are not a node's own */
    uint32_t pad_;
} mwhip_kernel_stat;
int32_t mwhip_profile(mwhip_exec *exec, uint64_t graph, uint32_t reps,
                      mwhip_kernel_stat *out, uint32_t max_out);

/* Snapshots: one saved copy of everything a step reads and an earlier step wrote
 * -- the live rows of every column of every table with numRows / needsSort /
 * sortedRows / tailRows and the per-world ranges, the entity slots in use, the
 * per-world id caches, idFreeHead / numIds / the run-time id partition, the
 * per-world data, tmpOffset and the persistent region up to persistOffset --
 * held in device memory that belongs to the executor.  One kernel launch per
 * save or restore (behind a one-workgroup prologue on save) moves the live rows
 * only; the row counts are read on the device, so the asynchronous forms are
 * stream-ordered behind the replays queued before them.  A snapshot can be
 * saved into and restored from any number of times, by the executor that made
 * it.  NOT rewound: the executor's replay counters (and with them the input
 * and output rings' slot position), errorFlags, capacities, and the ray caster's output
 * columns (derived state: they keep their contents until the next render
 * pass).  (No reference counterpart.)
 *
 * mwhip_snapshot_save waits for the stream, sizes the snapshot for the rows
 * mapped now, saves and waits again: it cannot overflow.
 * mwhip_snapshot_save_async keeps the size of the last synchronous save (or of
 * mwhip_snapshot_create): a table that has outgrown that room is not copied
 * and the snapshot is marked overflowed -- restoring it is refused until it has
 * been saved into again.
 * Errors (non-zero, text in mwhip_last_error(), state untouched): an unknown
 * handle or one of another executor, restoring a snapshot that was never saved,
 * restoring one whose last save overflowed. */
int mwhip_snapshot_create(mwhip_exec *exec, uint64_t *snapshot_out);
void mwhip_snapshot_destroy(mwhip_exec *exec, uint64_t snapshot);
int mwhip_snapshot_save(mwhip_exec *exec, uint64_t snapshot);
int mwhip_snapshot_restore(mwhip_exec *exec, uint64_t snapshot);
int mwhip_snapshot_save_async(mwhip_exec *exec, uint64_t snapshot);
int mwhip_snapshot_restore_async(mwhip_exec *exec, uint64_t snapshot);
/* bytes the last save holds (waits for the stream); 0: never saved / unknown */
uint64_t mwhip_snapshot_bytes(mwhip_exec *exec, uint64_t snapshot);
/* UNSTABLE, measurement only (profiles/tools/snapshot_time.py needs it for its
 * copy-per-segment yardstick): not part of what ABI 9 promises, may change or
 * go without a version bump, and hands out raw device addresses that the next
 * growth or sort invalidates -- do not build on it.  The segments of the last
 * save as (live address, address in the snapshot, bytes) triples, at most
 * max_out of them; returns how many there are.  Waits for the stream. */
typedef struct mwhip_snapshot_segment {
    void *live;
    void *saved;
    uint64_t num_bytes;
} mwhip_snapshot_segment;
int32_t mwhip_snapshot_segments(mwhip_exec *exec, uint64_t snapshot,
                                mwhip_snapshot_segment *out, uint32_t max_out);

/* State digests (added under ABI 9): D[g][w], a 64-bit hash per world w of a
 * chosen set of columns, computed by one kernel into a small device buffer
 * (madrona_amd/digest_ref.py is the same arithmetic in numpy).
 * A PLAN is an ordered list of columns (archetype_id, component_id), numbered
 * by position p = 0, 1, ...; Entity (component 0) and WorldID (component 1) may
 * be listed like any other.  The columns of one archetype form a GROUP (they
 * need not be adjacent in the plan); groups are ordered by their first column,
 * a group's tag t is the plan position of that column, and a group's columns
 * are taken in plan order.  All arithmetic is on uint64, modulo 2^64:
 *   K1 = 0x9E3779B97F4A7C15  K2 = 0xBF58476D1CE4E5B9  K3 = 0x94D049BB133111EB
 *   fin(x):       x ^= x >> 30; x *= K2; x ^= x >> 27; x *= K3; x ^= x >> 31
 *   absorb(h, v): h = (h ^ v) * K1;  h ^= h >> 32
 *   row(g, r):    h = fin(t_g + K1)
 *                 for each column c of group g, in plan order:
 *                     h = absorb(h, p_c)
 *                     for each little-endian 32-bit word v of the row's cell in
 *                             c (the cell zero-padded up to a multiple of 4 bytes):
 *                         h = absorb(h, v)
 *                 return fin(h)
 *   D[g][w] = sum of row(g, r) over the rows r < numRows of g's table whose
 *             WorldID == w
 * Rows destroyed in place (WorldID < 0) add nothing.  D[g][w] is a function of
 * the MULTISET of world w's rows in the table: it does not depend on where the
 * rows sit, on which side of a column's twin buffers is current, on other
 * worlds or on whether the table is sorted -- and it does not see the ORDER of
 * a world's rows.  A cell swapped between two rows of one world is seen (a
 * row's columns are chained).  Row counts and column addresses are read on the
 * device when the kernel runs, so the asynchronous form is stream-ordered behind
 * the replays queued before it, and a digest made before a table grew stays
 * valid.  The buffer is zeroed in the same stream-ordered sequence.
 *
 * mwhip_digest_buffer: device address of uint64 D[groups][worlds] (owned by the
 * executor, valid until the digest is destroyed), NULL for an unknown handle.
 * mwhip_digest_group: archetype id and tag of group `group`.
 * mwhip_set_step_digest: every replay of every STEP graph of the executor
 * (packed ones included; render graphs are untouched) recomputes that digest,
 * zeroing included, behind all of its task-graph nodes and before its pack node
 * and its output rings -- an output ring whose src is mwhip_digest_buffer() so
 * records the digest of step k in slot k.  0: none.  Lives in the executor, not
 * in a graph: waits for the stream and rebuilds the launch graphs (handles stay
 * valid; rebuilds on table growth keep it).  mwhip_profile lists the launches
 * with roles "digest.zero" and "digest"; the latter's algo_bytes are the bytes
 * of the listed cells of the live rows.  Destroying the step digest unsets it.
 * Handles are unique in the process; mwhip_destroy frees what is left.
 * Errors (non-zero, text in mwhip_last_error(), nothing changed): an unknown
 * handle or one of another executor ("digest N is not one of this executor's";
 * looked up first, so also with a null executor), n == 0, an archetype that is
 * not registered, a component the archetype does not have, the same column
 * listed twice, more than MWHIP_DIGEST_MAX_COLUMNS columns or
 * MWHIP_DIGEST_MAX_GROUPS groups.  (No reference counterpart.) */
#define MWHIP_DIGEST_MAX_COLUMNS 256
#define MWHIP_DIGEST_MAX_GROUPS 64
typedef struct mwhip_digest_column {
    uint32_t archetype_id;
    uint32_t component_id;
} mwhip_digest_column;
int mwhip_digest_create(mwhip_exec *exec, const mwhip_digest_column *columns,
                        uint32_t n, uint64_t *digest_out);
void mwhip_digest_destroy(mwhip_exec *exec, uint64_t digest);
/* waits for the executor's stream */
int mwhip_digest_compute(mwhip_exec *exec, uint64_t digest);
/* queued on the executor's stream behind the replays queued so far */
int mwhip_digest_compute_async(mwhip_exec *exec, uint64_t digest);
void *mwhip_digest_buffer(mwhip_exec *exec, uint64_t digest, uint32_t *groups_out,
                          uint32_t *worlds_out);
int mwhip_digest_group(mwhip_exec *exec, uint64_t digest, uint32_t group,
                       uint32_t *archetype_out, uint32_t *tag_out);
int mwhip_set_step_digest(mwhip_exec *exec, uint64_t digest);

/* World views (added under ABI 9): a dense, zero-padded, world-major copy of
 * chosen columns of ONE table, written by one kernel where the table is
 * (madrona_amd/view_ref.py is the same definition in numpy).
 * A view names one archetype a, an ordered list of n of its components and
 * max_rows >= 1; Entity (component 0) and WorldID (component 1) may be listed
 * like any other.  With W = the executor's number of worlds, a compute reads the
 * table's row count and column addresses on the device at the time the kernel
 * runs and leaves
 *   count[w]   (int32) the rows r < numRows of the table whose WorldID cell
 *              equals w: the full count, NOT clipped to max_rows;
 *   V_c[w][j]  for each listed column c, the cell of the j-th such row in table
 *              order (ascending r), for j < min(count[w], max_rows);
 *   zero bytes for every j from there up to max_rows.
 * So: every compute writes the buffers in full, padding included (what an
 * earlier compute or a caller left there never shows); rows beyond max_rows are
 * dropped, and count[w] > max_rows tells the caller that some were; rows
 * destroyed in place (WorldID < 0) belong to no world.  The result does not
 * depend on which side of a column's twin buffers is current, on whether
 * worldOffsets / worldCounts are current, or on whether the table has a sorted
 * prefix, holes in it, rows appended behind it, or was last sorted by another
 * key: a row is placed by its own WorldID cell.  After a full step of a
 * world-sorted table the view is the reference CPU backend's per-world table,
 * padded.  The asynchronous form is stream-ordered behind the replays queued
 * before it, and a view made before a table grew stays valid.
 *
 * mwhip_view_buffer: device address of uint8 V_c[W][max_rows][cell_bytes] of
 * listed column `column` (position in the list), 256-byte aligned, owned by the
 * executor and valid until the view is destroyed; NULL for an unknown handle or
 * a column index out of range.  mwhip_view_counts: int32 count[W], likewise.
 * mwhip_set_step_view(on != 0): every replay of every STEP graph of the
 * executor (packed ones included; render graphs are untouched) recomputes the
 * view behind all of its task-graph nodes (and behind the step digest) and
 * before its pack node and its output rings -- an output ring whose src is
 * mwhip_view_buffer() so records [K][W][max_rows][cell_bytes] of ragged data
 * with nothing but graph launches on the stream.  Up to MWHIP_MAX_STEP_VIEWS
 * step views, ONE launch for all of them; mwhip_profile lists it with role
 * "view", algo_bytes = bytes written (the buffers and counts in full) + bytes
 * read (the listed cells of the rows copied and the WorldID cell of every row
 * counted).  on == 0 takes it out again.  The set lives in the executor, not in
 * a graph: changing it waits for the stream and rebuilds the launch graphs
 * (handles stay valid; rebuilds on table growth keep it).  Destroying a step
 * view unsets it.  Views are derived state: snapshots do not save them (a
 * restore followed by a compute gives the restored worlds' view).  Handles are
 * unique in the process; mwhip_destroy frees what is left.
 * Errors (non-zero, text in mwhip_last_error(), nothing changed): an unknown
 * handle or one of another executor ("view N is not one of this executor's";
 * looked up first, so also with a null executor), n == 0 or
 * n > MWHIP_VIEW_MAX_COLUMNS, max_rows == 0, an archetype that is not
 * registered, a component the archetype does not have, a component listed
 * twice, a ninth step view, buffers that cannot be allocated.
 * (No reference counterpart.) */
#define MWHIP_VIEW_MAX_COLUMNS 32
#define MWHIP_MAX_STEP_VIEWS 8
int mwhip_view_create(mwhip_exec *exec, uint32_t archetype_id, const uint32_t *component_ids,
                      uint32_t n, uint32_t max_rows, uint64_t *view_out);
void mwhip_view_destroy(mwhip_exec *exec, uint64_t view);
/* waits for the executor's stream */
int mwhip_view_compute(mwhip_exec *exec, uint64_t view);
/* queued on the executor's stream behind the replays queued so far */
int mwhip_view_compute_async(mwhip_exec *exec, uint64_t view);
void *mwhip_view_buffer(mwhip_exec *exec, uint64_t view, uint32_t column,
                        uint64_t *bytes_out, uint32_t *cell_bytes_out);
int32_t *mwhip_view_counts(mwhip_exec *exec, uint64_t view);
int mwhip_set_step_view(mwhip_exec *exec, uint64_t view, int on);

/* World writes (added under ABI 9): the inverse of a world view.  Padded
 * per-world tensors are scattered into the rows of chosen columns of ONE table
 * by one kernel where the table is (madrona_amd/write_ref.py is
 * the same definition in numpy).  A write names one archetype a, an ordered
 * list of n of its components -- NOT Entity (component 0) or WorldID
 * (component 1) -- and max_rows >= 1, and owns, with W = the executor's number
 * of worlds,
 *   in_c   (in)  uint8 [W][max_rows][cell_bytes] per listed column c, 256-byte
 *                aligned: exactly the layout of a world view made with the same
 *                columns and max_rows, so what a view produced can be copied in
 *                tensor for tensor; the caller fills them;
 *   take   (in)  int32 [W]: how many leading rows of each world to write;
 *   count  (out) int32 [W]: each world's rows in the table, not clipped.
 * All of them are zero at creation: an apply before anything is filled writes
 * nothing.  An apply reads the table's row count and column addresses on the
 * device at the time the kernel runs and does, for every world w:
 *   count[w] = the rows r < numRows of the table whose WorldID cell equals w;
 *   k = min(max(take[w], 0), count[w], max_rows);
 *   for j < k, the listed cells of the j-th such row in table order (ascending
 *   r) become in_c[w][j].
 * Every other byte of the table is unchanged: rows of w from k on, rows
 * destroyed in place (WorldID < 0), unlisted columns, the Entity and WorldID
 * columns, the table header (numRows, needsSort, sortedRows, the world ranges).
 * in_c and take are not modified.  As for views, the result does not depend on
 * which side of a column's twin buffers is current, on whether worldOffsets /
 * worldCounts are current, or on whether the table has a sorted prefix, holes
 * in it, rows appended behind it, or was last sorted by another key: a row is
 * found by its own WorldID cell.  What a simulator derives from a written
 * component (a rigid body's broadphase leaf from its pose, say) is the
 * simulator's business, exactly as if one of its own systems had written the
 * component: it follows when the system that derives it next runs.  Filling
 * the buffers (from another stream, say) is ordered against an apply by the
 * caller, as for exported action tensors.  The asynchronous form is
 * stream-ordered behind the replays queued before it, and a write made before a
 * table grew stays valid.
 *
 * mwhip_write_buffer: device address of in_c of listed column `column`
 * (position in the list), owned by the executor and valid until the write is
 * destroyed; NULL for an unknown handle or a column index out of range.
 * mwhip_write_take / mwhip_write_counts: take and count, likewise.
 * mwhip_set_step_write(on != 0): every replay of every STEP graph of the
 * executor (packed ones included; render graphs are untouched) applies the
 * write directly behind its input-ring launches and in front of its first
 * task-graph node -- an input ring whose dst is mwhip_write_buffer() or
 * mwhip_write_take() so feeds the injection of the same replay, and K queued
 * steps carry K different injections with nothing but graph launches on the
 * stream.  Up to MWHIP_MAX_STEP_WRITES step writes, ONE launch for all of them;
 * mwhip_profile lists it with name and role "write", algo_bytes = rows written
 * x listed row bytes x 2 (read from the slab, written to the table) + 4 bytes
 * per WorldID cell counted, worked out after the run from take and count.
 * on == 0 takes it out again.  The set lives in the executor, not in a graph:
 * changing it waits for the stream and rebuilds the launch graphs (handles stay
 * valid; rebuilds on table growth keep it).  Destroying a step write unsets it.
 * Snapshots do not save a write's buffers.  Handles are unique in the process;
 * mwhip_destroy frees what is left.
 * Errors (non-zero, text in mwhip_last_error(), nothing changed or allocated):
 * an unknown handle or one of another executor ("write N is not one of this
 * executor's"; looked up first, so also with a null executor), n == 0 or
 * n > MWHIP_WRITE_MAX_COLUMNS, max_rows == 0, an archetype that is not
 * registered, a component the archetype does not have, a component listed
 * twice, the Entity or the WorldID column listed, a ninth step write, buffers
 * that cannot be allocated.
 * (No reference counterpart.) */
#define MWHIP_WRITE_MAX_COLUMNS 32
#define MWHIP_MAX_STEP_WRITES 8
int mwhip_write_create(mwhip_exec *exec, uint32_t archetype_id, const uint32_t *component_ids,
                       uint32_t n, uint32_t max_rows, uint64_t *write_out);
void mwhip_write_destroy(mwhip_exec *exec, uint64_t write);
/* waits for the executor's stream */
int mwhip_write_apply(mwhip_exec *exec, uint64_t write);
/* queued on the executor's stream behind the replays queued so far */
int mwhip_write_apply_async(mwhip_exec *exec, uint64_t write);
void *mwhip_write_buffer(mwhip_exec *exec, uint64_t write, uint32_t column,
                         uint64_t *bytes_out, uint32_t *cell_bytes_out);
int32_t *mwhip_write_take(mwhip_exec *exec, uint64_t write);
int32_t *mwhip_write_counts(mwhip_exec *exec, uint64_t write);
int mwhip_set_step_write(mwhip_exec *exec, uint64_t write, int on);

/* World reductions (added under ABI 9): one number per world, element and term
 * about ONE table, computed by one kernel where the table is (DESIGN.md §28;
 * madrona_amd/reduce_ref.py is the same definition in numpy).  A reduce names
 * one archetype a and an ordered list of n TERMS
 *   { component_id, byte_offset, num_elems, dtype, op, flags, limit }.
 * The same component may appear in several terms; Entity (component 0) and
 * WorldID (component 1) may be listed.
 * Rows and elements.  The rows of world w are the rows r < numRows of the
 * table whose WorldID cell equals w, taken in ascending r: exactly the world
 * view's rule.  Rows destroyed in place (WorldID < 0) belong to no world.
 * Nothing depends on which side of a column's twin buffers is current, on
 * worldOffsets / worldCounts being current, or on the sorted prefix.  Element
 * e < num_elems of row j is the `dtype` value at byte_offset + e *
 * sizeof(dtype) of that row's cell of the component (F32, I32, U32: 4 bytes,
 * U8: 1 byte).
 * Outputs, with W = the executor's number of worlds:
 *   count[w]   int32 [W]: the number of rows of w, as for views;
 *   R_t[w][e]  one 4-byte result [W][num_elems] per term t;
 *   alarm[w]   int32 [W], 0 or 1.
 * Operations, x_j being element e of the j-th row of w (row order):
 *   SUM             f32 / i32 / u32 (U8 widened to u32).  F32: acc = +0.0f,
 *                   then acc = acc + x_j in row order, fp32 round-to-nearest,
 *                   no reassociation, no flushing of denormals.  Integers:
 *                   modulo 2^32.
 *   MIN             as above.  acc = +inf (F32) or the largest value of the
 *                   result type; if (x < acc) acc = x in row order.  A NaN
 *                   never replaces; of -0 and +0 the first one met stays.
 *   MAX             mirrored: acc = -inf, INT32_MIN or 0; if (x > acc) acc = x.
 *   ABSMAX          F32 only, f32: acc = +0; a = x with the sign bit cleared;
 *                   if (a > acc) acc = a.  NaNs are ignored, Inf counts.
 *   COUNT_NONZERO   int32: the rows with x != 0.  NaN counts, -0 does not.
 *   COUNT_NONFINITE F32 only, int32: the rows whose exponent bits are all ones.
 * A world without rows gets the identities.
 * Alarms.  A term with MWHIP_REDUCE_ALARM in flags TRIPS for w when any of its
 * elements meets the condition: COUNT_*: the result is > 0; F32 ABSMAX and
 * MAX: the result is > limit; F32 MIN: the result is < limit.  alarm[w] = 1 if
 * any alarm term trips for w, else 0.  `limit` is ignored without the flag.
 * Every compute writes all outputs in full; they start as zeros; each is
 * 256-byte aligned and all sit in one allocation per reduce.  A compute reads
 * the table's row count, sorted prefix and column addresses on the device when
 * the kernel runs: the asynchronous form is stream-ordered behind the replays
 * queued before it, and a reduce made before a table grew stays valid.
 *
 * mwhip_reduce_buffer: device address of R_t of term `term` (position in the
 * list), valid until the reduce is destroyed; *bytes_out = W * num_elems * 4,
 * *elems_out = num_elems; NULL for an unknown handle or a term out of range.
 * mwhip_reduce_counts / mwhip_reduce_alarm: count and alarm, likewise.
 * mwhip_set_step_reduce(on != 0): every replay of every STEP graph of the
 * executor (packed ones included; render graphs are untouched) recomputes the
 * reduce behind its last task-graph node, its step digest and its step views
 * and in front of its pack node and its output-ring copies: an output ring
 * whose src is one of the buffers records one result per step, and an input
 * ring whose ring is mwhip_reduce_alarm() (one slot) feeds the alarm of replay
 * k to the head of replay k + 1 with nothing but graph launches on the stream.
 * Up to MWHIP_MAX_STEP_REDUCES step reduces, ONE launch for all of them;
 * mwhip_profile lists it with name and role "reduce", algo_bytes = the bytes
 * written + per row counted its WorldID cell and its listed elements, worked
 * out after the run from count.  on == 0 takes it out again.  The set lives in
 * the executor, not in a graph: changing it waits for the stream and rebuilds
 * the launch graphs (handles stay valid; rebuilds on table growth keep it).
 * Destroying a step reduce unsets it.  Snapshots do not save a reduce's
 * buffers.  Handles are unique in the process; mwhip_destroy frees what is left.
 * Errors (non-zero, text in mwhip_last_error(), nothing changed or allocated):
 * an unknown handle or one of another executor ("reduce N is not one of this
 * executor's"; looked up first, so also with a null executor), n == 0 or
 * n > MWHIP_REDUCE_MAX_TERMS, num_elems == 0, more than MWHIP_REDUCE_MAX_ELEMS
 * elements in all, an unknown dtype, op or flag, ABSMAX or COUNT_NONFINITE on a
 * dtype other than F32, the alarm flag on an (op, dtype) pair without a rule
 * above, an archetype that is not registered, a component the archetype does
 * not have, a byte_offset that is not a multiple of the element size, a cell
 * whose size is not, an element range that leaves the cell, a ninth step
 * reduce, buffers that cannot be allocated.
 * (No reference counterpart.) */
#define MWHIP_REDUCE_MAX_TERMS 32
#define MWHIP_REDUCE_MAX_ELEMS 256
#define MWHIP_MAX_STEP_REDUCES 8
#define MWHIP_REDUCE_F32 0u
#define MWHIP_REDUCE_I32 1u
#define MWHIP_REDUCE_U32 2u
#define MWHIP_REDUCE_U8 3u
#define MWHIP_REDUCE_SUM 0u
#define MWHIP_REDUCE_MIN 1u
#define MWHIP_REDUCE_MAX 2u
#define MWHIP_REDUCE_ABSMAX 3u
#define MWHIP_REDUCE_COUNT_NONZERO 4u
#define MWHIP_REDUCE_COUNT_NONFINITE 5u
#define MWHIP_REDUCE_ALARM 1u
typedef struct mwhip_reduce_term {
    uint32_t component_id;
    uint32_t byte_offset;   /* of element 0 in the component's cell */
    uint32_t num_elems;
    uint32_t dtype;         /* MWHIP_REDUCE_F32 .. _U8 */
    uint32_t op;            /* MWHIP_REDUCE_SUM .. _COUNT_NONFINITE */
    uint32_t flags;         /* MWHIP_REDUCE_ALARM or 0 */
    float limit;            /* of an F32 ABSMAX / MAX / MIN alarm */
} mwhip_reduce_term;
int mwhip_reduce_create(mwhip_exec *exec, uint32_t archetype_id, const mwhip_reduce_term *terms,
                        uint32_t n, uint64_t *reduce_out);
void mwhip_reduce_destroy(mwhip_exec *exec, uint64_t reduce);
/* waits for the executor's stream */
int mwhip_reduce_compute(mwhip_exec *exec, uint64_t reduce);
/* queued on the executor's stream behind the replays queued so far */
int mwhip_reduce_compute_async(mwhip_exec *exec, uint64_t reduce);
void *mwhip_reduce_buffer(mwhip_exec *exec, uint64_t reduce, uint32_t term,
                          uint64_t *bytes_out, uint32_t *elems_out);
int32_t *mwhip_reduce_counts(mwhip_exec *exec, uint64_t reduce);
int32_t *mwhip_reduce_alarm(mwhip_exec *exec, uint64_t reduce);
int mwhip_set_step_reduce(mwhip_exec *exec, uint64_t reduce, int on);

/* Entity gathers (added under ABI 9): N entity handles read from device memory
 * turned into, per listed component, the cell the entity each handle names
 * has, plus where that entity lives, by one kernel that goes through the
 * entity store as Context::get<T>(e) does (DESIGN.md §31;
 * madrona_amd/gather_ref.py is the same definition in numpy).
 * The SOURCE is a run of records: num_records records of record_bytes each
 * from src on, and in each record handles_per_record consecutive 8-byte Entity
 * cells ({ uint32 gen; int32 id }) from byte first_byte on.  N = num_records *
 * handles_per_record; handle i is read at
 *   src + (i / handles_per_record) * record_bytes + first_byte
 *       + (i % handles_per_record) * 8.
 * A handle h NAMES row r of table a exactly when h.id >= 0, a is a registered
 * archetype, 0 <= r < numRows(a), the Entity cell of that row (column 0) equals
 * h bit for bit and the row's WorldID cell (column 1) is not -1.  (A row
 * destroyed in place and a temporary's row hold Entity::none(), id -1: a
 * negative id names nothing.)  Such a row is unique if it exists.  A compute leaves
 *   archetype[i]  (int32) a, or -1 when handle i names nothing;
 *   world[i]      (int32) that row's WorldID cell, or -1 likewise;
 *   G_c[i]        for each listed component c, the row's cell of c; all zero
 *                 when handle i names nothing or table a has no column of c.
 * Every byte of every output is rewritten by every compute.  Handles are
 * arbitrary bits (a stale generation, Entity::none(), an id nobody has, zero
 * padding, anything a caller wrote): the kernel dereferences nothing behind a
 * check that failed.  Row counts, column addresses, the entity store's size
 * and the handles themselves are read on the device when the kernel runs: a
 * gather made before a table or the entity store grew, or before a sort
 * swapped a column with its twin, stays right.  n == 0 is allowed (only
 * archetype and world are produced); Entity (component 0) and WorldID
 * (component 1) may be listed like any other component.
 *
 * src is the caller's: it must be 4-byte aligned and stay valid and in place
 * while the gather exists.  An exported tensor (pinned), a world view's slab
 * (mwhip_view_buffer), a gather's own buffer, any device allocation are valid
 * sources.  A table column's own address is NOT: the sort swaps a column with
 * its twin.  To read a column of handles, make a world view of it and gather
 * through the view's slab (handles_per_record > 1 and first_byte address
 * handles inside wider cells, e.g. Entity buttons[4] of a 40-byte cell).
 *
 * mwhip_gather_buffer: device address of uint8 G_c[N][cell_bytes] of listed
 * component `column` (position in the list), 256-byte aligned, owned by the
 * executor and valid until the gather is destroyed; NULL for an unknown handle
 * or a column index out of range.  mwhip_gather_archetypes / mwhip_gather_worlds:
 * int32 [N], likewise.
 * mwhip_set_step_gather(on != 0): every replay of every STEP graph of the
 * executor (packed ones included; render graphs are untouched) recomputes the
 * gather directly behind the step views -- so a gather may read a step view's
 * slab of the same replay -- and before the step reduces, the pack node and
 * the output rings: a step view of a handle column, a step gather over its
 * slab and an output ring over mwhip_gather_buffer() record
 * [K][W][rows][handles][cell_bytes] of referenced entities with nothing but
 * graph launches on the stream.  Up to MWHIP_MAX_STEP_GATHERS step gathers,
 * ONE launch for all of them; mwhip_profile lists it with role "gather",
 * algo_bytes = bytes written (the buffers, archetype and world in full) +
 * bytes read (the handles, and per handle that named an entity its slot, its
 * row's Entity and WorldID cells and the listed cells).  on == 0 takes it out
 * again.  The set lives in the executor, not in a graph: changing it waits for
 * the stream and rebuilds the launch graphs (handles stay valid).  Destroying a
 * step gather unsets it.  Gathers are derived state: snapshots do not save
 * them (a restore followed by a compute gives the restored worlds' gather).
 * Handles are unique in the process; mwhip_destroy frees what is left.
 * Errors (non-zero, text in mwhip_last_error(), nothing changed or allocated):
 * -3 for an unknown handle or one of another executor ("gather N is not one of
 * this executor's"; looked up first, so also with a null executor); -2 for a
 * null src, src / record_bytes / first_byte not a multiple of 4,
 * handles_per_record == 0, first_byte + 8 * handles_per_record > record_bytes,
 * num_records == 0, N > 2^31 - 1, n > MWHIP_GATHER_MAX_COLUMNS, a component
 * that is not registered, a component listed twice, a ninth step gather; -10
 * for buffers that cannot be allocated.
 * (No reference counterpart.) */
#define MWHIP_GATHER_MAX_COLUMNS 32
#define MWHIP_MAX_STEP_GATHERS 8
typedef struct mwhip_gather_source {
    const void *src;                /* device address of record 0 */
    uint64_t num_records;
    uint32_t record_bytes;
    uint32_t first_byte;            /* of handle 0 inside a record */
    uint32_t handles_per_record;
    uint32_t pad_;
} mwhip_gather_source;
int mwhip_gather_create(mwhip_exec *exec, const mwhip_gather_source *source,
                        const uint32_t *component_ids, uint32_t n, uint64_t *gather_out);
void mwhip_gather_destroy(mwhip_exec *exec, uint64_t gather);
/* waits for the executor's stream */
int mwhip_gather_compute(mwhip_exec *exec, uint64_t gather);
/* queued on the executor's stream behind the replays queued so far */
int mwhip_gather_compute_async(mwhip_exec *exec, uint64_t gather);
void *mwhip_gather_buffer(mwhip_exec *exec, uint64_t gather, uint32_t column,
                          uint64_t *bytes_out, uint32_t *cell_bytes_out);
int32_t *mwhip_gather_archetypes(mwhip_exec *exec, uint64_t gather);
int32_t *mwhip_gather_worlds(mwhip_exec *exec, uint64_t gather);
int mwhip_set_step_gather(mwhip_exec *exec, uint64_t gather, int on);

/* Entity scatters (added under ABI 9): the batched ctx.get<T>(e) = v, the other
 * direction of an entity gather (madrona_amd/scatter_ref.py is
 * the same definition in numpy).  The SOURCE of the N handles is a
 * mwhip_gather_source, read and checked exactly as a gather's: the same
 * alignment rules, the same definition of "handle i NAMES row r of table a"
 * (id >= 0, a registered, 0 <= r < numRows(a), the row's Entity cell equal to
 * the handle bit for bit, its WorldID cell not -1), and the same warning that a
 * table column's own address is no source.  A scatter owns, all zero at creation,
 *   in_c[i]       (uint8 [N][cell_bytes], in) per listed component c;
 *   select[i]     (int32 [N], in);
 *   archetype[i], world[i], written[i]   (int32 [N], out).
 * An apply is the sequential loop for i = 0 .. N - 1: if select[i] != 0 and
 * handle i names (a, r), then for every listed component c that table a has a
 * column of, that column's cell of row r becomes in_c[i].  So among selected
 * handles that name the same entity THE HIGHEST INDEX WINS, whatever the
 * scheduling.  Every apply rewrites in full
 *   archetype[i], world[i]   as a gather does: -1, -1 when handle i names
 *                 nothing, whatever select says;
 *   written[i]    1 exactly when select[i] != 0, handle i names an entity and
 *                 no selected handle of higher index names the same entity
 *                 (also when the table has none of the listed columns), else 0.
 * Every other byte of every table is unchanged: unlisted columns, Entity and
 * WorldID (which cannot be listed), the headers, the rows of handles that lost,
 * were not selected or name nothing.  The buffers, select and the source are
 * not modified.  No rows are created or destroyed, and state derived from the
 * cells written is the simulator's business, as for a world write.  Handles are
 * arbitrary bits: nothing is dereferenced behind a check that failed, and a
 * cell is stored only behind the full check of its own handle.  Row counts,
 * column addresses and the entity store's size are read on the device when
 * the kernels run: a scatter made before a table or the entity store grew, or
 * before a sort swapped a column with its twin, stays right.
 *
 * An apply is three launches ordered by the stream: one clears the scatter's
 * claim table (slots = the power of two >= 2N, at most 2^31; uint32 keys[slots],
 * entity id + 1, and uint32 best[slots], handle index + 1), one resolves every
 * handle, stores archetype and world and claims the entity for the highest
 * selected index (compare-and-swap, atomic max), one resolves again, stores
 * written and copies the winners' cells.  No workgroup waits for another.
 *
 * mwhip_scatter_buffer: device address of in_c of listed component `column`
 * (position in the list), 256-byte aligned, owned by the executor and valid
 * until the scatter is destroyed; NULL for an unknown handle or a column index
 * out of range.  mwhip_scatter_select / _archetypes / _worlds / _written: int32
 * [N], likewise.  One allocation holds all of them and the claim table.
 * mwhip_set_step_scatter(on != 0): every replay of every STEP graph of the
 * executor (packed ones included; render graphs are untouched) applies the
 * scatter directly behind the step writes and in front of the first task-graph
 * node, so an input ring whose destination is a buffer, select or a handle
 * tensor of the caller's feeds the apply of the replay it runs in.  Up to
 * MWHIP_MAX_STEP_SCATTERS step scatters, THREE launches for all of them (each
 * scatter has its own claim table in them); mwhip_profile lists them with
 * roles "scatter.zero", "scatter.claim" and "scatter.write"; algo_bytes: the
 * claim tables; per handle 20 bytes (handle, select, archetype, world) + per
 * handle that named an entity 24 (its slot, its row's Entity and WorldID
 * cells); per handle 16 (handle, select, written) + per named handle 24 + per
 * winner twice the listed cells.  Two step scatters could name one entity in
 * one launch: a scatter that lists a component which a set step scatter already
 * lists is refused (distinct components are distinct columns).  The step writes
 * run one launch earlier: on the same cell a step scatter wins over a step
 * write.  A step scatter over a step view's slab reads the view the PREVIOUS
 * replay left, which is the state this replay starts from.  While a step
 * scatter is set, replays run every launch (no carried broadphase).  on == 0
 * takes it out again; changing the set waits for the stream and rebuilds the
 * launch graphs (handles stay valid).  Destroying a step scatter unsets it.
 * Handles are unique in the process; mwhip_destroy frees what is left.
 * Errors (non-zero, text in mwhip_last_error(), nothing changed or allocated):
 * -3 for an unknown handle or one of another executor ("scatter N is not one
 * of this executor's"; looked up first, so also with a null executor); -2 for
 * everything mwhip_gather_create refuses about a source and a component list
 * (n > MWHIP_SCATTER_MAX_COLUMNS), n == 0, the Entity (0) or WorldID (1)
 * component listed, a ninth step scatter, a component clash among step
 * scatters; -10 for buffers that cannot be allocated.
 * (No reference counterpart.) */
#define MWHIP_SCATTER_MAX_COLUMNS 32
#define MWHIP_MAX_STEP_SCATTERS 8
int mwhip_scatter_create(mwhip_exec *exec, const mwhip_gather_source *source,
                         const uint32_t *component_ids, uint32_t n, uint64_t *scatter_out);
void mwhip_scatter_destroy(mwhip_exec *exec, uint64_t scatter);
/* waits for the executor's stream */
int mwhip_scatter_apply(mwhip_exec *exec, uint64_t scatter);
/* queued on the executor's stream behind the replays queued so far */
int mwhip_scatter_apply_async(mwhip_exec *exec, uint64_t scatter);
void *mwhip_scatter_buffer(mwhip_exec *exec, uint64_t scatter, uint32_t column,
                           uint64_t *bytes_out, uint32_t *cell_bytes_out);
int32_t *mwhip_scatter_select(mwhip_exec *exec, uint64_t scatter);
int32_t *mwhip_scatter_archetypes(mwhip_exec *exec, uint64_t scatter);
int32_t *mwhip_scatter_worlds(mwhip_exec *exec, uint64_t scatter);
int32_t *mwhip_scatter_written(mwhip_exec *exec, uint64_t scatter);
int mwhip_set_step_scatter(mwhip_exec *exec, uint64_t scatter, int on);

/* Ray queries (added under ABI 9): N = F x R rays -- F fans of R >= 1 rays that
 * share an origin and a world -- cast through the worlds' broadphase BVHs
 * (broadphase::BVH::traceRay / traceRayShared, <madrona/broadphase.hpp>) by one
 * kernel, the batched form of what a lidar system does (DESIGN.md §33;
 * madrona_amd/ray_ref.py is the same definition in numpy).  Ray i = f * R + r
 * is ray r of fan f.
 * INPUTS.  world, count and origin are each either a buffer the query owns or
 * a SOURCE of the caller's, mwhip_ray_source: record k is read at
 * src + k * record_bytes + first_byte; src, record_bytes and first_byte are
 * multiples of 4; the source is read on the device when the kernel runs and
 * must stay valid and in place while the query exists (an exported tensor, a
 * world view's slab or counts, any device allocation; NOT a table column's own
 * address, which the sort swaps with its twin -- as for a gather).  Owned
 * buffers are 256-byte aligned and zero at creation (t_max: +inf); the caller
 * and input rings write them.
 *   world[f]    int32 per fan.  fans_per_world > 0 replaces it by the rule
 *               world = f / fans_per_world (the shape of a world view's slab):
 *               desc.world is then ignored and no world buffer is owned.
 *   count[w]    optional int32 per WORLD (desc.count.src != NULL; e.g. a
 *               view's counts), only with fans_per_world > 0: fan f with
 *               f % fans_per_world >= count[world] is SKIPPED.
 *   origin[f]   3 floats per fan (possibly inside a wider record).
 *   dir[i]      3 floats per ray, always owned, used as given: hit_t is in
 *               units of its length, as in traceRay.
 *   t_max[i]    float per ray, always owned.
 * OUTPUTS, owned, every one rewritten in full by every compute, valid until
 * the query is destroyed:
 *   status[i]   int32: MWHIP_RAYS_HIT 1, MWHIP_RAYS_MISS 0, MWHIP_RAYS_SKIPPED
 *               -1, MWHIP_RAYS_BAD_WORLD -2 (world not in [0, numWorlds)),
 *               MWHIP_RAYS_BAD_RAY -3 (a non-finite component of origin or
 *               direction, an all-zero direction, a NaN t_max).  Checked in that
 *               order: world, count, origin (per fan), then direction and t_max
 *               (per ray).  Nothing behind a failed check is read: no count of a
 *               bad world, no origin of a skipped fan, no tree for a negative
 *               status.
 *   hit_t[i]    float, 0 on anything but a HIT;
 *   hit[i]      8 bytes, Entity { uint32 gen; int32 id }, Entity::none()
 *               (0xFFFFFFFF, -1) on anything but a HIT: the buffer is a valid
 *               mwhip_gather_source with record_bytes 8;
 *   normal[i]   3 floats, zero on anything but a HIT.
 * A ray sees the tree as the LAST BROADPHASE PASS left it (the precondition of
 * BVH::traceRay: leaf boxes are refreshed by PhysicsSystem::setupBroadphaseTasks,
 * not by writes to Position); spheres are transparent, as in traceRayIntoLeaf.
 * A world whose tree NO broadphase pass has built yet -- before the first step,
 * or restored from a snapshot taken then -- holds nothing a ray could meet:
 * its rays are MISS and the tree's memory is not touched.  (While a rebuild of
 * a built tree is pending, a ray walks the old tree, as BVH::traceRay does.)
 *
 * THE KERNEL lives in the simulator's code object (the physics headers,
 * phys_impl/ray_query.inl), because traceRayShared and its LDS scratch do:
 * PhysicsSystem::setupBroadphaseTasks hands its host stub over with
 * mwhip_set_ray_kernel (NULL is ignored).  Its single argument is a
 * mwhip_ray_args by value, whose plans (mwhip_ray_plan, device-resident) the
 * runtime fills: both code objects compile these two structs from this header.
 * A work item is a wavefront = two groups of 32 lanes.  rays_per_fan >= 8
 * (groups_per_fan = ceil(R / 32) > 0): a group holds up to 32 rays of ONE fan
 * and goes through traceRayShared; smaller R (groups_per_fan == 0): rays are
 * packed one per lane through plain traceRay.  Same bits either way.  A simulator
 * that registered none (no broadphase) has no ray queries.
 *
 * mwhip_rays_buffer: device address and size of owned buffer `which`
 * (MWHIP_RAYS_BUF_*); NULL (-2) for world / origin when a source was given (or
 * fans_per_world > 0), NULL (-3) for an unknown handle.
 * mwhip_set_step_rays(on != 0): every replay of every STEP graph recomputes the
 * query behind the step views (origins and counts may be a step view's of the
 * same replay) and in front of the step gathers (a step gather over `hit` sees
 * this replay's hits), the step reduces, the pack node and the output rings (a
 * ring over an output records [K][N]...).  Up to MWHIP_MAX_STEP_RAYS, ONE launch
 * for all, listed by mwhip_profile as "rays" with role "rays"; none when none
 * is set.  Changing the set waits for the stream and rebuilds the launch graphs;
 * destroying a step query unsets it.  Ray queries are derived state: snapshots
 * do not save them.
 * Errors (non-zero, text in mwhip_last_error(), nothing changed or allocated):
 * -3 for an unknown handle or one of another executor ("ray query N is not one
 * of this executor's"; looked up first, so also with a null executor); -2 for
 * no registered kernel ("this simulator registered no ray kernel"), num_fans ==
 * 0, rays_per_fan == 0, F x R > 2^31 - 1, a source whose src / record_bytes /
 * first_byte is not a multiple of 4 or whose record is too short for its item,
 * a count source without fans_per_world, a fifth step query; -10 for buffers
 * that cannot be allocated.
 * (No reference counterpart.) */
#define MWHIP_MAX_STEP_RAYS 4
#define MWHIP_RAYS_HIT 1
#define MWHIP_RAYS_MISS 0
#define MWHIP_RAYS_SKIPPED (-1)
#define MWHIP_RAYS_BAD_WORLD (-2)
#define MWHIP_RAYS_BAD_RAY (-3)
#define MWHIP_RAYS_BUF_WORLD 0u
#define MWHIP_RAYS_BUF_ORIGIN 1u
#define MWHIP_RAYS_BUF_DIR 2u
#define MWHIP_RAYS_BUF_T_MAX 3u
#define MWHIP_RAYS_BUF_HIT_T 4u
#define MWHIP_RAYS_BUF_HIT 5u
#define MWHIP_RAYS_BUF_NORMAL 6u
#define MWHIP_RAYS_BUF_STATUS 7u
#define MWHIP_RAYS_NUM_BUFS 8u
typedef struct mwhip_ray_source {
    const void *src;                /* device address of record 0; NULL: none */
    uint32_t record_bytes;
    uint32_t first_byte;            /* of the item inside a record */
} mwhip_ray_source;
typedef struct mwhip_rays_desc {
    uint32_t num_fans;              /* F */
    uint32_t rays_per_fan;          /* R >= 1 */
    uint32_t fans_per_world;        /* > 0: world[f] = f / fans_per_world */
    uint32_t pad_;
    mwhip_ray_source world;         /* src == NULL: an owned buffer */
    mwhip_ray_source count;         /* src == NULL: no counts */
    mwhip_ray_source origin;        /* src == NULL: an owned buffer */
} mwhip_rays_desc;
/* what the kernel reads of one query (device-resident, filled by the runtime;
 * first_byte is already added to the three sources) */
typedef struct mwhip_ray_plan {
    void *state;                    /* the executor's ecs state on the device */
    const char *world_src;          /* unused when fans_per_world > 0 */
    const char *count_src;          /* NULL: none */
    const char *origin_src;
    const float *dir;               /* [N][3] */
    const float *t_max;             /* [N] */
    float *hit_t;                   /* [N] */
    uint32_t *hit;                  /* [N][2] */
    float *normal;                  /* [N][3] */
    int32_t *status;                /* [N] */
    uint32_t world_stride, count_stride, origin_stride;     /* bytes */
    uint32_t num_fans, rays_per_fan, fans_per_world;
    uint32_t groups_per_fan;        /* 0: packed, a ray per lane */
    uint32_t pad_;
} mwhip_ray_plan;
/* the kernel's argument, by value: items[p] wavefronts work on plans[p] */
typedef struct mwhip_ray_args {
    uint32_t num_plans;
    uint32_t pad_;
    uint32_t items[MWHIP_MAX_STEP_RAYS];
    const mwhip_ray_plan *plans[MWHIP_MAX_STEP_RAYS];
} mwhip_ray_args;
/* the simulator's ray kernel: __global__ void(mwhip_ray_args), 256 threads */
int mwhip_set_ray_kernel(mwhip_exec *exec, const void *kernel);
int mwhip_rays_create(mwhip_exec *exec, const mwhip_rays_desc *desc, uint64_t *rays_out);
void mwhip_rays_destroy(mwhip_exec *exec, uint64_t rays);
/* waits for the executor's stream */
int mwhip_rays_compute(mwhip_exec *exec, uint64_t rays);
/* queued on the executor's stream behind the replays queued so far */
int mwhip_rays_compute_async(mwhip_exec *exec, uint64_t rays);
void *mwhip_rays_buffer(mwhip_exec *exec, uint64_t rays, uint32_t which, uint64_t *bytes_out);
int mwhip_set_step_rays(mwhip_exec *exec, uint64_t rays, int on);

/* Box queries (added under ABI 9): B = F x G boxes -- F bundles of G >= 1 boxes
 * that share a world and a centre -- tested through the worlds' broadphase BVHs
 * by one kernel, the batched form of PhysicsSystem::findEntitiesWithinAABB
 * (<madrona/physics.hpp>): per box the WHOLE list of the entities that call
 * reports, in the order it reports them (madrona_amd/box_ref.py
 * is the same definition in numpy).  Box b = f * G + g is box g of bundle f:
 *     pMin = centre[f] + lo[b],  pMax = centre[f] + hi[b]      (float32)
 * INPUTS.  world, count and centre are each either a buffer the query owns or a
 * SOURCE of the caller's, a mwhip_ray_source with a ray query's rules (record k
 * at src + k * record_bytes + first_byte, multiples of 4, read on the device
 * when the kernel runs, in place while the query exists).  Owned buffers are
 * 256-byte aligned and zero at creation: every box starts empty, and with an
 * owned centre lo and hi are absolute corners.
 *   world[f]    int32 per bundle.  bundles_per_world > 0 replaces it by the rule
 *               world = f / bundles_per_world: desc.world is then ignored and no
 *               world buffer is owned.
 *   count[w]    optional int32 per WORLD, only with bundles_per_world > 0:
 *               bundle f with f % bundles_per_world >= count[world] is SKIPPED.
 *   centre[f]   3 floats per bundle (possibly inside a wider record).
 *   lo[b], hi[b]  3 floats per box each, always owned.
 * OUTPUTS, owned, every one rewritten in full by every compute:
 *   status[b]   int32: MWHIP_BOXES_OK 0, MWHIP_BOXES_SKIPPED -1,
 *               MWHIP_BOXES_BAD_WORLD -2 (world not in [0, numWorlds)),
 *               MWHIP_BOXES_BAD_BOX -3 (a non-finite component of centre, lo, hi
 *               or of a sum, or pMin > pMax on an axis).  Checked in that order:
 *               world, count, centre (per bundle), then per box.  Nothing behind
 *               a failed check is read.
 *   count[b]    int32: how many entities findEntitiesWithinAABB(ctx of world,
 *               box, fn) reports; NOT capped by max_hits; 0 unless OK.
 *   hits[b][k]  k < max_hits, 8 bytes each, Entity { uint32 gen; int32 id }: the
 *               first min(count, max_hits) entities in report order,
 *               Entity::none() behind them: the buffer is a valid
 *               mwhip_gather_source of B x max_hits handles, record_bytes 8.
 * A box sees the tree as the LAST BROADPHASE PASS left it and the bodies' poses
 * as they are now, the precondition of a simulator's own node that calls
 * findEntitiesWithinAABB.  A world whose tree NO broadphase pass has built yet
 * (numNodes() == 0) gives OK with count 0, its tree untouched.  While a rebuild
 * of a built tree is pending the old tree is walked, as findEntitiesWithinAABB
 * does.
 *
 * THE KERNEL lives in the simulator's code object (phys_impl/box_query.inl):
 * PhysicsSystem::setupBroadphaseTasks hands its host stub over with
 * mwhip_set_box_kernel (NULL is ignored).  Its single argument is a
 * mwhip_box_args by value whose plans (mwhip_box_plan, device-resident) the
 * runtime fills.  Two mappings that leave the same words.  Cooperative (the
 * default): a group of 32 lanes, two per wavefront, owns a chunk of up to 32
 * boxes of ONE bundle and enumerates the tree's leaves in traversal order, 32
 * per window, sharing the box-independent half of the hull test.  Packed
 * (MWHIP_BOXES_PACKED in desc.flags): a box per lane through plain
 * findEntitiesWithinAABB.  items[p] counts wavefronts either way.
 *
 * mwhip_boxes_buffer: device address and size of owned buffer `which`
 * (MWHIP_BOXES_BUF_*); NULL (-2) for world / centre when a source was given (or
 * bundles_per_world > 0), NULL (-3) for an unknown handle.
 * mwhip_set_step_boxes(on != 0): every replay of every STEP graph recomputes the
 * query directly behind the step ray queries and in front of the step gathers:
 * centres and counts may be a step view's of the same replay, a step gather over
 * `hits` sees this replay's hits, an output ring over count or hits records
 * [K]...  Up to MWHIP_MAX_STEP_BOXES, ONE launch for all, listed by
 * mwhip_profile as "boxes" with role "boxes"; none when none is set.  Changing
 * the set waits for the stream and rebuilds the launch graphs; destroying a step
 * query unsets it.  Box queries are derived state: snapshots do not save them.
 * Errors (non-zero, text in mwhip_last_error(), nothing changed or allocated):
 * -3 for an unknown handle or one of another executor (also with a null
 * executor); -2 for no registered kernel ("this simulator registered no box
 * kernel"), num_bundles == 0, boxes_per_bundle == 0, max_hits == 0, B x
 * max_hits > 2^31 - 1, an unknown flag, a bad source (as for rays), a count
 * source without bundles_per_world, a fifth step query; -10 for buffers that
 * cannot be allocated.
 * (No reference counterpart.) */
#define MWHIP_MAX_STEP_BOXES 4
#define MWHIP_BOXES_OK 0
#define MWHIP_BOXES_SKIPPED (-1)
#define MWHIP_BOXES_BAD_WORLD (-2)
#define MWHIP_BOXES_BAD_BOX (-3)
#define MWHIP_BOXES_PACKED 1u          /* mwhip_boxes_desc::flags */
#define MWHIP_BOXES_BUF_WORLD 0u
#define MWHIP_BOXES_BUF_CENTRE 1u
#define MWHIP_BOXES_BUF_LO 2u
#define MWHIP_BOXES_BUF_HI 3u
#define MWHIP_BOXES_BUF_STATUS 4u
#define MWHIP_BOXES_BUF_COUNT 5u
#define MWHIP_BOXES_BUF_HITS 6u
#define MWHIP_BOXES_NUM_BUFS 7u
typedef struct mwhip_boxes_desc {
    uint32_t num_bundles;           /* F */
    uint32_t boxes_per_bundle;      /* G >= 1 */
    uint32_t max_hits;              /* K >= 1 */
    uint32_t bundles_per_world;     /* > 0: world[f] = f / bundles_per_world */
    uint32_t flags;                 /* MWHIP_BOXES_PACKED */
    uint32_t pad_;
    mwhip_ray_source world;         /* src == NULL: an owned buffer */
    mwhip_ray_source count;         /* src == NULL: no counts */
    mwhip_ray_source centre;        /* src == NULL: an owned buffer */
} mwhip_boxes_desc;
/* what the kernel reads of one query (device-resident, filled by the runtime;
 * first_byte is already added to the three sources) */
typedef struct mwhip_box_plan {
    void *state;                    /* the executor's ecs state on the device */
    const char *world_src;          /* unused when bundles_per_world > 0 */
    const char *count_src;          /* NULL: none */
    const char *centre_src;
    const float *lo;                /* [B][3] */
    const float *hi;                /* [B][3] */
    int32_t *status;                /* [B] */
    int32_t *count;                 /* [B] */
    uint32_t *hits;                 /* [B][K][2] */
    uint32_t world_stride, count_stride, centre_stride;     /* bytes */
    uint32_t num_bundles, boxes_per_bundle, max_hits, bundles_per_world;
    uint32_t chunks_per_bundle;     /* ceil(G / 32); 0: packed, a box per lane */
} mwhip_box_plan;
/* the kernel's argument, by value: items[p] wavefronts work on plans[p] */
typedef struct mwhip_box_args {
    uint32_t num_plans;
    uint32_t pad_;
    uint32_t items[MWHIP_MAX_STEP_BOXES];
    const mwhip_box_plan *plans[MWHIP_MAX_STEP_BOXES];
} mwhip_box_args;
/* the simulator's box kernel: __global__ void(mwhip_box_args), 256 threads */
int mwhip_set_box_kernel(mwhip_exec *exec, const void *kernel);
int mwhip_boxes_create(mwhip_exec *exec, const mwhip_boxes_desc *desc, uint64_t *boxes_out);
void mwhip_boxes_destroy(mwhip_exec *exec, uint64_t boxes);
/* waits for the executor's stream */
int mwhip_boxes_compute(mwhip_exec *exec, uint64_t boxes);
/* queued on the executor's stream behind the replays queued so far */
int mwhip_boxes_compute_async(mwhip_exec *exec, uint64_t boxes);
void *mwhip_boxes_buffer(mwhip_exec *exec, uint64_t boxes, uint32_t which, uint64_t *bytes_out);
int mwhip_set_step_boxes(mwhip_exec *exec, uint64_t boxes, int on);

/* Contact queries (added under ABI 9): per world the primitive pairs of its
 * rigid bodies that TOUCH, with the manifold the narrowphase of the physics step
 * builds for each -- which bodies, where, how deep (DESIGN.md §36;
 * madrona_amd/contact_ref.py is the same definition in numpy with the
 * narrowphase injected).  The step drops its contacts inside its kernel; this
 * query runs the same narrowphase again, from outside.
 * WHICH PAIRS.  The bodies of world w are the rows of the rigid-body archetypes
 * in the step's iteration order, k = 0 .. n - 1.  Every pair k_lo < k_hi that is
 * not Static-Static, and of it every primitive pair (aPrim, bPrim) of the two
 * objects, where body `a` is the one with the LOWER ENTITY ID (as the step's
 * broadphase assigns it); the pair is then ordered by primitive type as the step
 * orders it.  A primitive pair is a contact iff the world boxes of the two
 * primitives intersect (the step's own test) and the narrowphase returns a
 * manifold with at least one point.  No BVH is involved: the result is a
 * function of the tables alone.
 * ORDER: ascending (k_lo, k_hi, aPrim * b_num_prims + bPrim).
 * POSES.  Default: the SOLVER POSES, position and rotation of a body's
 * xpbd::PreSolvePositional -- the poses the solver's last substep built its
 * contacts at, where a resting body penetrates by about g h^2 instead of 0 +- an
 * ulp; a body whose stored rotation is exactly (0, 0, 0, 0), never stepped since
 * it was created, is taken at its current pose.  MWHIP_CONTACTS_CURRENT_POSES:
 * Position and Rotation as they are now.  Scale, ObjectID and ResponseType are
 * always the current ones.
 * INPUT.  select[w], optional int32 per world: 0 skips the world.  Either a
 * buffer the query owns (desc.own_select != 0; 1 at creation) or a SOURCE of the
 * caller's, a mwhip_ray_source with a ray query's rules; neither: every world.
 * OUTPUTS, owned, 256-byte aligned, every one rewritten in full by every compute
 * (K = max_contacts):
 *   status[w]        int32: MWHIP_CONTACTS_OK 0, MWHIP_CONTACTS_SKIPPED -1
 *                    (select[w] == 0), MWHIP_CONTACTS_UNSORTED -2 (a rigid-body
 *                    table waits for its world sort: no world has a row range),
 *                    MWHIP_CONTACTS_UNSUPPORTED -3 (a primitive pair no path
 *                    supports).  No sticky error flag is raised.
 *   count[w]         int32: the world's contacts, NOT capped by K; 0 unless OK.
 *   pairs[w][k][2]   Entity { uint32 gen; int32 id } x 2: the body that owns the
 *                    reference feature, then the other (a reference face's body;
 *                    `a` for an edge contact; the plane; of a sphere pair `b`).
 *                    Entity::none() behind min(count, K): a valid
 *                    mwhip_gather_source of W x K x 2 handles, record_bytes 8.
 *   num_points[w][k] int32, 1 .. 4
 *   normal[w][k][3]  float32
 *   points[w][k][4][4]  float32: xyz world position, w penetration depth; point
 *                    slots >= num_points are zero.
 *                    All three zero behind min(count, K).
 * THE KERNEL lives in the simulator's code object
 * (phys_impl/contact_query.inl): PhysicsSystem::setupPhysicsStepTasks hands its
 * host stub over with mwhip_set_contact_kernel (NULL is ignored); caps bit 0
 * (MWHIP_CONTACT_CAP_SOLVER_POSES): the simulator's bodies have solver poses
 * (XPBD).  Its single argument is a mwhip_contact_args by value.  A wavefront per
 * world.  Two mappings that leave the same words: cooperative (the default: the
 * step kernel's narrowphase on chunks of 64 pairs whose boxes intersect) and
 * MWHIP_CONTACTS_PLAIN (every such pair through the generic single-lane
 * routine, the definition itself).
 * mwhip_set_step_contacts(on != 0): every replay of every STEP graph recomputes
 * the query directly behind the step box queries and in front of the step
 * gathers (which may read `pairs`).  Up to MWHIP_MAX_STEP_CONTACTS, ONE launch
 * for all, listed by mwhip_profile as "contacts" with role "contacts"; none when
 * none is set.  Destroying a step query unsets it.  Contact queries are derived
 * state: snapshots do not save them.
 * Errors (non-zero, text in mwhip_last_error(), nothing changed or allocated):
 * -3 for an unknown handle or one of another executor; -2 for no registered
 * kernel, solver poses asked of a simulator without them ("this simulator has
 * no solver poses"), max_contacts == 0, W x K x 2 > 2^31 - 1, an unknown flag,
 * a bad source (as for rays; also a source together with own_select), a fifth
 * step query; -10 for buffers that cannot be allocated.
 * (No reference counterpart: the reference clears its contacts every substep.) */
#define MWHIP_MAX_STEP_CONTACTS 4
#define MWHIP_CONTACTS_OK 0
#define MWHIP_CONTACTS_SKIPPED (-1)
#define MWHIP_CONTACTS_UNSORTED (-2)
#define MWHIP_CONTACTS_UNSUPPORTED (-3)
#define MWHIP_CONTACTS_CURRENT_POSES 1u     /* mwhip_contacts_desc::flags */
#define MWHIP_CONTACTS_PLAIN 2u
#define MWHIP_CONTACT_CAP_SOLVER_POSES 1u   /* mwhip_set_contact_kernel caps */
#define MWHIP_CONTACTS_BUF_SELECT 0u
#define MWHIP_CONTACTS_BUF_STATUS 1u
#define MWHIP_CONTACTS_BUF_COUNT 2u
#define MWHIP_CONTACTS_BUF_PAIRS 3u
#define MWHIP_CONTACTS_BUF_NUM_POINTS 4u
#define MWHIP_CONTACTS_BUF_NORMAL 5u
#define MWHIP_CONTACTS_BUF_POINTS 6u
#define MWHIP_CONTACTS_NUM_BUFS 7u
typedef struct mwhip_contacts_desc {
    uint32_t max_contacts;          /* K >= 1 */
    uint32_t flags;                 /* MWHIP_CONTACTS_CURRENT_POSES | _PLAIN */
    uint32_t own_select;            /* != 0: an owned select buffer */
    uint32_t pad_;
    mwhip_ray_source select;        /* src == NULL: none (or the owned one) */
} mwhip_contacts_desc;
/* what the kernel reads of one query (device-resident, filled by the runtime;
 * first_byte is already added to the source) */
typedef struct mwhip_contact_plan {
    void *state;                    /* the executor's ecs state on the device */
    const char *select_src;         /* NULL: every world */
    int32_t *status;                /* [W] */
    int32_t *count;                 /* [W] */
    uint32_t *pairs;                /* [W][K][2][2] */
    int32_t *num_points;            /* [W][K] */
    float *normal;                  /* [W][K][3] */
    float *points;                  /* [W][K][4][4] */
    uint32_t select_stride;         /* bytes */
    uint32_t max_contacts, flags, num_worlds;
} mwhip_contact_plan;
/* the kernel's argument, by value: a wavefront serves world w of every plan,
 * one plan after the other; items[p] == the number of worlds */
typedef struct mwhip_contact_args {
    uint32_t num_plans;
    uint32_t pad_;
    uint32_t items[MWHIP_MAX_STEP_CONTACTS];
    const mwhip_contact_plan *plans[MWHIP_MAX_STEP_CONTACTS];
} mwhip_contact_args;
/* the simulator's contact kernel: __global__ void(mwhip_contact_args), 256 threads */
int mwhip_set_contact_kernel(mwhip_exec *exec, const void *kernel, uint32_t caps);
int mwhip_contacts_create(mwhip_exec *exec, const mwhip_contacts_desc *desc,
                          uint64_t *contacts_out);
void mwhip_contacts_destroy(mwhip_exec *exec, uint64_t contacts);
/* waits for the executor's stream */
int mwhip_contacts_compute(mwhip_exec *exec, uint64_t contacts);
/* queued on the executor's stream behind the replays queued so far */
int mwhip_contacts_compute_async(mwhip_exec *exec, uint64_t contacts);
void *mwhip_contacts_buffer(mwhip_exec *exec, uint64_t contacts, uint32_t which,
                            uint64_t *bytes_out);
int mwhip_set_step_contacts(mwhip_exec *exec, uint64_t contacts, int on);

/* Shape queries (added under ABI 9): S = F x G posed collision shapes, F bundles
 * of G shapes that share a world, each tested against the rigid bodies of its
 * world with the narrowphase of the physics step -- "if this object stood THERE,
 * what would it touch, where, and how deep?" (DESIGN.md §39;
 * madrona_amd/shape_ref.py is the same definition in numpy with the narrowphase
 * injected).  Shape s = f * G + g is shape g of bundle f.
 * INPUTS.  world[f] int32 per bundle, count[w] int32 per WORLD (only with
 * bundles_per_world > 0: world = f / bundles_per_world, and bundle f with
 * f % bundles_per_world >= count[world] is SKIPPED) and exclude[s], one Entity
 * { uint32 gen; int32 id } per shape, are each a buffer the query owns (world,
 * exclude) or a SOURCE of the caller's, a mwhip_ray_source with a ray query's
 * rules; count is a source or nothing.  A body whose Entity column equals
 * exclude[s], gen and id both, is not tested against shape s; Entity::none()
 * excludes nothing.  Always owned: object[s] int32 (an object of the
 * ObjectManager, < desc.num_objects -- the manager keeps no count on the
 * device, so num_objects >= 1 is the caller's statement of how many it holds),
 * position[s] 3 floats, rotation[s] 4 floats (w, x, y, z), scale[s] 3 floats.
 * At creation object is 0, position 0, rotation (1, 0, 0, 0), scale 1, exclude
 * none, world 0.
 * WHAT IS TESTED.  The bodies of the shape's world are the rows of the
 * rigid-body archetypes in the step's iteration order, k = 0 .. n - 1, at their
 * CURRENT Position, Rotation and Scale.  Every body that is not excluded, Static
 * ones included, and of it every primitive pair c = shapePrim * body_num_prims +
 * bodyPrim.  The shape is argument `a` of the step's pair setup, which then
 * orders the two by primitive type.  The pair is a hit iff the world boxes of
 * the two primitives intersect (the step's own test) and the narrowphase returns
 * a manifold of at least one point.  ORDER: ascending (k, c).  No BVH is walked:
 * the result is a function of the tables and the inputs alone.
 * OUTPUTS, owned, 256-byte aligned, every one rewritten in full by every compute
 * (K = max_hits):
 *   status[s]        int32: MWHIP_SHAPES_OK 0, _SKIPPED -1, _BAD_WORLD -2 (world
 *                    outside [0, W)), _BAD_SHAPE -3 (a non-finite component of
 *                    position, rotation or scale, or an object outside [0,
 *                    num_objects)), _UNSORTED -4 (a rigid-body table waits for
 *                    its world sort), _UNSUPPORTED -5 (a primitive pair no path
 *                    supports).  Checked in the order world, count, then per
 *                    shape; nothing behind a failed check is read.  No sticky
 *                    error flag is raised.
 *   count[s]         int32: hits, NOT capped by K; 0 unless OK.
 *   hits[s][k]       Entity of the body touched; Entity::none() behind
 *                    min(count, K): a valid mwhip_gather_source of S x K handles,
 *                    record_bytes 8.
 *   shape_is_ref[s][k] int32: 1 where the contact's reference side
 *                    (ContactConstraint::ref) is the shape, else 0.  The normal
 *                    points away from the reference side: out of the shape where
 *                    1, out of the body (towards the shape) where 0 -- a
 *                    reference face's or the plane's outward normal, away from
 *                    `a` for an edge contact, from the hull to the sphere.  The
 *                    one exception is a sphere-sphere pair, whose normal points
 *                    from `a` to the reference `b`.
 *   num_points[s][k] int32, 1 .. 4
 *   normal[s][k][3]  float32
 *   points[s][k][4][4]  float32: xyz world position, w penetration depth; point
 *                    slots >= num_points are zero.
 *                    All four zero behind min(count, K).
 * THE KERNEL lives in the simulator's code object (phys_impl/shape_query.inl):
 * PhysicsSystem::setupPhysicsStepTasks hands its host stub over with
 * mwhip_set_shape_kernel (NULL is ignored) together with the bytes of HBM
 * scratch a wavefront needs for the generic single-lane routine (0 with a
 * kernel: -2).  The executor
 * owns ONE block of that many bytes per wavefront of the largest grid, made by
 * the first create and shared by all shape queries (computes are
 * stream-ordered).  Its single argument is a mwhip_shape_args by value.  A
 * wavefront per bundle.  Two mappings that leave the same words: cooperative
 * (the default) and MWHIP_SHAPES_PLAIN (every pair whose boxes intersect
 * through the generic single-lane routine, the definition itself).
 * mwhip_set_step_shapes(on != 0): every replay of every STEP graph recomputes
 * the query directly behind the step contact queries and in front of the step
 * gathers (which may read `hits`).  Up to MWHIP_MAX_STEP_SHAPES, ONE launch for
 * all, listed by mwhip_profile as "shapes" with role "shapes"; none when none is
 * set.  Destroying a step query unsets it.  Shape queries are derived state:
 * snapshots do not save them.
 * Errors (non-zero, text in mwhip_last_error(), nothing changed or allocated):
 * -3 for an unknown handle or one of another executor; -2 for no registered
 * kernel, num_bundles, shapes_per_bundle, max_hits or num_objects of 0, S x K >
 * 2^31 - 1, an unknown flag, a bad source (as for rays), a count source without
 * bundles_per_world, a fifth step query; -10 for buffers that cannot be
 * allocated.
 * (No reference counterpart.) */
#define MWHIP_MAX_STEP_SHAPES 4
#define MWHIP_SHAPES_OK 0
#define MWHIP_SHAPES_SKIPPED (-1)
#define MWHIP_SHAPES_BAD_WORLD (-2)
#define MWHIP_SHAPES_BAD_SHAPE (-3)
#define MWHIP_SHAPES_UNSORTED (-4)
#define MWHIP_SHAPES_UNSUPPORTED (-5)
#define MWHIP_SHAPES_PLAIN 1u               /* mwhip_shapes_desc::flags */
#define MWHIP_SHAPES_BUF_WORLD 0u
#define MWHIP_SHAPES_BUF_EXCLUDE 1u
#define MWHIP_SHAPES_BUF_OBJECT 2u
#define MWHIP_SHAPES_BUF_POSITION 3u
#define MWHIP_SHAPES_BUF_ROTATION 4u
#define MWHIP_SHAPES_BUF_SCALE 5u
#define MWHIP_SHAPES_BUF_STATUS 6u
#define MWHIP_SHAPES_BUF_COUNT 7u
#define MWHIP_SHAPES_BUF_HITS 8u
#define MWHIP_SHAPES_BUF_SHAPE_IS_REF 9u
#define MWHIP_SHAPES_BUF_NUM_POINTS 10u
#define MWHIP_SHAPES_BUF_NORMAL 11u
#define MWHIP_SHAPES_BUF_POINTS 12u
#define MWHIP_SHAPES_NUM_BUFS 13u
typedef struct mwhip_shapes_desc {
    uint32_t num_bundles;           /* F >= 1 */
    uint32_t shapes_per_bundle;     /* G >= 1 */
    uint32_t max_hits;              /* K >= 1 */
    uint32_t num_objects;           /* >= 1: the objects the ObjectManager holds */
    uint32_t bundles_per_world;     /* > 0: world = f / bundles_per_world */
    uint32_t flags;                 /* MWHIP_SHAPES_PLAIN */
    mwhip_ray_source world;         /* src == NULL: the owned buffer (or the rule) */
    mwhip_ray_source count;         /* src == NULL: every bundle */
    mwhip_ray_source exclude;       /* src == NULL: the owned buffer */
} mwhip_shapes_desc;
/* what the kernel reads of one query (device-resident, filled by the runtime;
 * first_byte is already added to the sources) */
typedef struct mwhip_shape_plan {
    void *state;                    /* the executor's ecs state on the device */
    const char *world_src;          /* unused with bundles_per_world > 0 */
    const char *count_src;          /* NULL: every bundle */
    const char *exclude_src;
    const int32_t *object;          /* [S] */
    const float *position;          /* [S][3] */
    const float *rotation;          /* [S][4] */
    const float *scale;             /* [S][3] */
    int32_t *status;                /* [S] */
    int32_t *count;                 /* [S] */
    uint32_t *hits;                 /* [S][K][2] */
    int32_t *shape_is_ref;          /* [S][K] */
    int32_t *num_points;            /* [S][K] */
    float *normal;                  /* [S][K][3] */
    float *points;                  /* [S][K][4][4] */
    char *scratch;                  /* scratch_waves x scratch_stride bytes */
    uint32_t world_stride, count_stride, exclude_stride;   /* bytes */
    uint32_t num_bundles, shapes_per_bundle, max_hits, num_objects, bundles_per_world, flags;
    uint32_t scratch_stride;        /* bytes per wavefront */
    uint32_t scratch_waves;         /* wavefronts the block serves */
    uint32_t pad_;
} mwhip_shape_plan;
/* the kernel's argument, by value: wavefronts stride over the bundles of all
 * plans, plan after plan; items[p] == plan p's bundles */
typedef struct mwhip_shape_args {
    uint32_t num_plans;
    uint32_t pad_;
    uint32_t items[MWHIP_MAX_STEP_SHAPES];
    const mwhip_shape_plan *plans[MWHIP_MAX_STEP_SHAPES];
} mwhip_shape_args;
/* the simulator's shape kernel: __global__ void(mwhip_shape_args), 256 threads */
int mwhip_set_shape_kernel(mwhip_exec *exec, const void *kernel,
                           uint32_t scratch_bytes_per_wavefront);
int mwhip_shapes_create(mwhip_exec *exec, const mwhip_shapes_desc *desc, uint64_t *shapes_out);
void mwhip_shapes_destroy(mwhip_exec *exec, uint64_t shapes);
/* waits for the executor's stream */
int mwhip_shapes_compute(mwhip_exec *exec, uint64_t shapes);
/* queued on the executor's stream behind the replays queued so far */
int mwhip_shapes_compute_async(mwhip_exec *exec, uint64_t shapes);
void *mwhip_shapes_buffer(mwhip_exec *exec, uint64_t shapes, uint32_t which, uint64_t *bytes_out);
int mwhip_set_step_shapes(mwhip_exec *exec, uint64_t shapes, int on);

#ifdef __cplusplus
}
#endif
#endif /* MWHIP_H */
