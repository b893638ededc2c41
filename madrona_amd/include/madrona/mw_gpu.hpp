// Host-side executor of the MI355X backend.
//
// API contract: reference include/madrona/mw_gpu.hpp:25-164 -- StateConfig,
// CompileConfig, MWCudaLaunchGraph and MWCudaExecutor keep their names,
// fields and method signatures so a simulator's Manager compiles unchanged
// ("Cuda" in the names is historical: everything below drives HIP).  The
// class is a header-only shim over the C ABI in include/mwhip.h; errors abort
// like the reference's REQ_CUDA / FATAL.
//
// Differences that are visible to callers:
//  * CompileConfig::userSources / userCompileFlags are accepted and ignored:
//    simulator device code is compiled offline by hipcc into the same shared
//    object; there is no runtime compiler.
//  * initCUDA returns an opaque context value carrying the gpu id.
#pragma once

#include <madrona/macros.hpp>
#include <madrona/span.hpp>
#include <madrona/optional.hpp>
#include <madrona/types.hpp>
#include <madrona/math.hpp>
#include <madrona/render/cuda_batch_render_assets.hpp>
#include <madrona/py/utils.hpp>

#include <mwhip.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

// Defined by MADRONA_BUILD_MWGPU_ENTRY in the simulator's device TU.
extern "C" const mwhip_user_entry *madronaMWHipUserEntry();

namespace madrona {

struct StateConfig {
    void *worldInitPtr;
    uint32_t numWorldInitBytes;
    void *userConfigPtr;
    uint32_t numUserConfigBytes;
    uint32_t numWorldDataBytes;
    uint32_t worldDataAlignment;
    uint32_t numWorlds;
    uint32_t numTaskGraphs;
    uint32_t numExportedBuffers;
};

struct CompileConfig {
    enum class OptMode : uint32_t {
        Optimize,
        LTO,
        Debug,
    };

    Span<const char *const> userSources;
    Span<const char *const> userCompileFlags;
    OptMode optMode = OptMode::LTO;
};

// Batch ray caster configuration (reference mw_gpu.hpp:77-96).  Geometry and
// materials arrive either in the reference's own form -- geoBVHData /
// materialData, the types of <madrona/render/cuda_batch_render_assets.hpp>:
// 4-wide quantised mesh BVHs with de-indexed vertices, per-triangle materials
// and texture objects, as a renderer's asset processor produces them -- or, for
// applications without such a processor (it needs Embree), as plain indexed
// triangles: geoTriangles / triangleMaterials, an addition of this backend.
// Either way the executor builds its own bottom-level trees from the triangles
// (any valid BVH gives the same image); of a MeshBVHData it reads the leaves.
namespace render {

// indexed triangles of the renderable objects, host memory
struct TriangleMeshData {
    Span<const math::Vector3> vertices = {};        // all objects
    Span<const uint32_t> indices = {};              // 3 per triangle, object-local
    Span<const uint32_t> objectVertexOffsets = {};  // [numObjects + 1]
    Span<const uint32_t> objectTriangleOffsets = {};// [numObjects + 1]
    Span<const math::Vector2> vertexUVs = {};       // per vertex, or empty
    // per triangle (all objects): the material of triangles of objects whose
    // objectMaterials entry is -1 (reference MeshBVH::leafMats); or empty
    Span<const int32_t> triangleMaterials = {};
};

struct TriangleMaterialData {
    Span<const math::Vector3> materialColors = {};
    Span<const int32_t> objectMaterials = {};       // [numObjects], -1: per triangle / none
    Span<const int32_t> materialTextures = {};      // per material: texture or -1; or empty
    Span<const TextureRGBA8> textures = {};
};

}

struct CudaBatchRenderConfig {
    enum class RenderMode : uint32_t {
        RGBD,
        Depth,
    };

    RenderMode renderMode = RenderMode::RGBD;
    render::MeshBVHData geoBVHData = {};
    render::MaterialData materialData = {};
    // 6 floats per object id (min xyz, max xyz), host memory; empty: taken from
    // the geometry
    Span<const float> objectRootAABBs = {};
    // the ray caster's outputs are renderResolution x renderResolution
    uint32_t renderResolution = 0;
    // (reference mw_gpu.hpp:89-90.  Its ray caster hands nearPlane down as
    // BVHParams::nearSphere -> TraceInfo::tMin, bvh_raycast.cpp:983, and never
    // reads tMin again: accepted here, with the same effect)
    float nearPlane = 0.f;
    float farPlane = 0.f;
    // ---- this backend ----
    // most views a world will hold, 0 = unknown: sizes the render-target table,
    // 8 * renderResolution^2 bytes a view
    uint32_t maxViewsPerWorld = 0;
    // the geometry as plain triangles (used when geoBVHData holds no meshes)
    render::TriangleMeshData geoTriangles = {};
    render::TriangleMaterialData triangleMaterials = {};
    // entries of materialData.materials (the reference's struct carries no
    // count); 0: one past the largest material id the meshes name
    uint32_t numMaterials = 0;
};

// Opaque device context handle (the reference returns a CUcontext)
struct MWHipContext {
    int32_t gpuID;
};
using CUcontext = MWHipContext;

class MWCudaExecutor;

class MWCudaLaunchGraph {
public:
    MWCudaLaunchGraph() : exec_(nullptr), graph_(0) {}
    MWCudaLaunchGraph(const MWCudaLaunchGraph &) = delete;
    MWCudaLaunchGraph(MWCudaLaunchGraph &&o) : exec_(o.exec_), graph_(o.graph_)
    {
        o.exec_ = nullptr;
        o.graph_ = 0;
    }

    ~MWCudaLaunchGraph()
    {
        if (exec_ != nullptr) {
            mwhip_free_launch_graph(exec_, graph_);
        }
    }

    MWCudaLaunchGraph &operator=(MWCudaLaunchGraph &&o)
    {
        if (this != &o) {
            if (exec_ != nullptr) {
                mwhip_free_launch_graph(exec_, graph_);
            }
            exec_ = o.exec_;
            graph_ = o.graph_;
            o.exec_ = nullptr;
            o.graph_ = 0;
        }
        return *this;
    }

    uint64_t handle() const { return graph_; }

private:
    MWCudaLaunchGraph(mwhip_exec *exec, uint64_t graph)
        : exec_(exec), graph_(graph)
    {}

    mwhip_exec *exec_;
    uint64_t graph_;

friend class MWCudaExecutor;
};

namespace detail {

// What MWHipSnapshot, MWHipDigest, MWHipWorldView, MWHipWorldWrite,
// MWHipWorldReduce, MWHipEntityGather, MWHipEntityScatter, MWHipRayQuery,
// MWHipBoxQuery, MWHipContactQuery and MWHipShapeQuery share: the move-only handle
// of an object that belongs to an executor (mwhip_<kind>_create / _destroy,
// include/mwhip.h), the device its buffers are on, and how one of those
// buffers becomes a py::Tensor.  Kind: { name, destroy(exec, handle) }.
template <typename Kind>
class ExecObject {
public:
    ExecObject() : exec_(nullptr), handle_(0), gpu_id_(0) {}
    ExecObject(const ExecObject &) = delete;
    ExecObject(ExecObject &&o) : exec_(o.exec_), handle_(o.handle_), gpu_id_(o.gpu_id_)
    {
        o.exec_ = nullptr;
        o.handle_ = 0;
    }

    ~ExecObject()
    {
        if (exec_ != nullptr) {
            Kind::destroy(exec_, handle_);
        }
    }

    ExecObject &operator=(ExecObject &&o)
    {
        if (this != &o) {
            if (exec_ != nullptr) {
                Kind::destroy(exec_, handle_);
            }
            exec_ = o.exec_;
            handle_ = o.handle_;
            gpu_id_ = o.gpu_id_;
            o.exec_ = nullptr;
            o.handle_ = 0;
        }
        return *this;
    }

    uint64_t handle() const { return handle_; }

protected:
    ExecObject(mwhip_exec *exec, uint64_t handle, int32_t gpu_id)
        : exec_(exec), handle_(handle), gpu_id_(gpu_id)
    {}

    static void req(int rc, const char *what)
    {
        if (rc != 0) {
            fprintf(stderr, "madrona_amd: %s %s failed (%d): %s\n", Kind::name, what, rc,
                    mwhip_last_error());
            abort();
        }
    }

    using Elem = py::TensorElementType;

    // one of the object's device buffers (nullptr: the runtime refused, and
    // member `what` fails) as a tensor of up to three dimensions
    py::Tensor tensor(void *ptr, Elem type, std::initializer_list<uint64_t> dims,
                      const char *what) const
    {
        req(ptr != nullptr ? 0 : -1, what);
        int64_t shape[3] = {};
        CountT n = 0;
        for (uint64_t d : dims) {
            shape[n++] = (int64_t)d;
        }
        return py::Tensor(ptr, type, Span<const int64_t>(shape, n),
                          Optional<int>::make((int)gpu_id_));
    }

    uint64_t numWorlds() const { return mwhip_num_worlds(exec_); }

    mwhip_exec *exec_;
    uint64_t handle_;
    int32_t gpu_id_;
};

struct SnapshotKind {
    static constexpr const char *name = "snapshot";
    static void destroy(mwhip_exec *exec, uint64_t handle) { mwhip_snapshot_destroy(exec, handle); }
};
struct DigestKind {
    static constexpr const char *name = "digest";
    static void destroy(mwhip_exec *exec, uint64_t handle) { mwhip_digest_destroy(exec, handle); }
};
struct WorldViewKind {
    static constexpr const char *name = "world view";
    static void destroy(mwhip_exec *exec, uint64_t handle) { mwhip_view_destroy(exec, handle); }
};
struct WorldWriteKind {
    static constexpr const char *name = "world write";
    static void destroy(mwhip_exec *exec, uint64_t handle) { mwhip_write_destroy(exec, handle); }
};
struct WorldReduceKind {
    static constexpr const char *name = "world reduce";
    static void destroy(mwhip_exec *exec, uint64_t handle) { mwhip_reduce_destroy(exec, handle); }
};
struct EntityGatherKind {
    static constexpr const char *name = "entity gather";
    static void destroy(mwhip_exec *exec, uint64_t handle) { mwhip_gather_destroy(exec, handle); }
};
struct EntityScatterKind {
    static constexpr const char *name = "entity scatter";
    static void destroy(mwhip_exec *exec, uint64_t handle) { mwhip_scatter_destroy(exec, handle); }
};
struct RayQueryKind {
    static constexpr const char *name = "ray query";
    static void destroy(mwhip_exec *exec, uint64_t handle) { mwhip_rays_destroy(exec, handle); }
};
struct BoxQueryKind {
    static constexpr const char *name = "box query";
    static void destroy(mwhip_exec *exec, uint64_t handle) { mwhip_boxes_destroy(exec, handle); }
};
struct ContactQueryKind {
    static constexpr const char *name = "contact query";
    static void destroy(mwhip_exec *exec, uint64_t handle) { mwhip_contacts_destroy(exec, handle); }
};
struct ShapeQueryKind {
    static constexpr const char *name = "shape query";
    static void destroy(mwhip_exec *exec, uint64_t handle) { mwhip_shapes_destroy(exec, handle); }
};

}

// Everything a batch of worlds is -- tables, entity store, per-world data, the
// persistent region -- saved in device memory and put back, any number of times
// (mwhip_snapshot_*, include/mwhip.h).  An extension of this backend: the
// reference leaves checkpoints to each simulator.  Not rewound: the executor's
// replay count (and the slot position of the input and output rings with it) and the ray
// caster's output columns, which keep their contents until the next render
// pass.  Belongs to the executor that made it and must not outlive it.
class MWHipSnapshot : public detail::ExecObject<detail::SnapshotKind> {
public:
    MWHipSnapshot() = default;

    // wait for the executor's stream; save() makes room for every row mapped
    void save() { req(mwhip_snapshot_save(exec_, handle_), "save"); }
    void restore() { req(mwhip_snapshot_restore(exec_, handle_), "restore"); }
    // queued on the executor's stream behind the replays queued so far
    void saveAsync() { req(mwhip_snapshot_save_async(exec_, handle_), "saveAsync"); }
    void restoreAsync()
    {
        req(mwhip_snapshot_restore_async(exec_, handle_), "restoreAsync");
    }
    // bytes the last save holds
    uint64_t numBytes() const { return mwhip_snapshot_bytes(exec_, handle_); }

private:
    MWHipSnapshot(mwhip_exec *exec, uint64_t snapshot, int32_t gpu_id)
        : ExecObject(exec, snapshot, gpu_id)
    {}

friend class MWCudaExecutor;
};

// One column of a digest's plan: (archetype id, component id), e.g.
// { TypeTracker::typeID<Agent>(), TypeTracker::typeID<Position>() }.
struct DigestColumn {
    uint32_t archetypeID;
    uint32_t componentID;
};
static_assert(sizeof(DigestColumn) == sizeof(mwhip_digest_column));

// A 64-bit hash per world of a chosen list of columns, one row of them per
// table the list names, computed by one kernel into a device buffer
// uint64 [numGroups()][worlds] (mwhip_digest_*, include/mwhip.h: the exact
// definition).  It is a hash of the multiset of each world's rows: blind to the
// order of a world's rows, to where they sit and to other worlds.  An extension
// of this backend.  Belongs to the executor that made it and must not outlive it.
class MWHipDigest : public detail::ExecObject<detail::DigestKind> {
public:
    MWHipDigest() = default;

    // waits for the executor's stream
    void compute() { req(mwhip_digest_compute(exec_, handle_), "compute"); }
    // queued on the executor's stream behind the replays queued so far
    void computeAsync() { req(mwhip_digest_compute_async(exec_, handle_), "computeAsync"); }
    // uint64 [numGroups()][worlds] on the device, owned by the executor
    void *devicePtr() const { return mwhip_digest_buffer(exec_, handle_, nullptr, nullptr); }
    uint32_t numGroups() const
    {
        uint32_t groups = 0;
        (void)mwhip_digest_buffer(exec_, handle_, &groups, nullptr);
        return groups;
    }

private:
    MWHipDigest(mwhip_exec *exec, uint64_t digest, int32_t gpu_id)
        : ExecObject(exec, digest, gpu_id)
    {}

friend class MWCudaExecutor;
};

// A dense, zero-padded, world-major copy of chosen columns of one table:
// per listed column uint8 [worlds][maxRows()][cell bytes] on the device, plus
// int32 [worlds] row counts (not clipped to maxRows()), written in full by one
// kernel where the table is, sorted or not (mwhip_view_*, include/mwhip.h: the
// exact definition).  An extension of this backend.  Belongs to the executor
// that made it and must not outlive it.
class MWHipWorldView : public detail::ExecObject<detail::WorldViewKind> {
public:
    MWHipWorldView() : max_rows_(0) {}

    // waits for the executor's stream
    void compute() { req(mwhip_view_compute(exec_, handle_), "compute"); }
    // queued on the executor's stream behind the replays queued so far
    void computeAsync() { req(mwhip_view_compute_async(exec_, handle_), "computeAsync"); }

    // uint8 [worlds][maxRows()][cell bytes] of listed column `column`
    // (position in the list given to makeWorldView), owned by the executor
    py::Tensor columnTensor(uint32_t column) const
    {
        uint64_t bytes = 0;
        uint32_t cell = 0;
        void *ptr = mwhip_view_buffer(exec_, handle_, column, &bytes, &cell);
        return tensor(ptr, Elem::UInt8, { numWorlds(), max_rows_, cell }, "columnTensor");
    }

    // int32 [worlds]: each world's rows in the table (may exceed maxRows())
    py::Tensor countsTensor() const
    {
        return tensor(mwhip_view_counts(exec_, handle_), Elem::Int32,
                      { numWorlds() }, "countsTensor");
    }

    uint32_t maxRows() const { return max_rows_; }

private:
    MWHipWorldView(mwhip_exec *exec, uint64_t view, uint32_t max_rows, int32_t gpu_id)
        : ExecObject(exec, view, gpu_id), max_rows_(max_rows)
    {}

    uint32_t max_rows_;

friend class MWCudaExecutor;
};

// The inverse of a world view: per listed column uint8 [worlds][maxRows()][cell
// bytes] on the device (the layout of a view of the same columns and maxRows())
// and int32 [worlds] `take`, both filled by the caller; apply() makes the
// listed cells of the first min(max(take[w], 0), rows of w, maxRows()) rows of
// every world w, in table order, those of the tensors, with one kernel where
// the table is, sorted or not, and leaves each world's row count (not clipped)
// in the counts (mwhip_write_*, include/mwhip.h: the exact definition).
// Nothing else of the table changes; what the simulator derives from the
// written components follows when its own systems next derive it.  Filling the
// tensors is ordered against apply by the caller, as for exported action
// tensors.  An extension of this backend.  Belongs to the executor that made
// it and must not outlive it.
class MWHipWorldWrite : public detail::ExecObject<detail::WorldWriteKind> {
public:
    MWHipWorldWrite() : max_rows_(0) {}

    // waits for the executor's stream
    void apply() { req(mwhip_write_apply(exec_, handle_), "apply"); }
    // queued on the executor's stream behind the replays queued so far
    void applyAsync() { req(mwhip_write_apply_async(exec_, handle_), "applyAsync"); }

    // uint8 [worlds][maxRows()][cell bytes] of listed column `column`
    // (position in the list given to makeWorldWrite), owned by the executor
    py::Tensor columnTensor(uint32_t column) const
    {
        uint64_t bytes = 0;
        uint32_t cell = 0;
        void *ptr = mwhip_write_buffer(exec_, handle_, column, &bytes, &cell);
        return tensor(ptr, Elem::UInt8, { numWorlds(), max_rows_, cell }, "columnTensor");
    }

    // int32 [worlds], in: the leading rows of each world to write
    py::Tensor takeTensor() const
    {
        return tensor(mwhip_write_take(exec_, handle_), Elem::Int32, { numWorlds() }, "takeTensor");
    }

    // int32 [worlds], out: each world's rows in the table (may exceed maxRows())
    py::Tensor countsTensor() const
    {
        return tensor(mwhip_write_counts(exec_, handle_), Elem::Int32,
                      { numWorlds() }, "countsTensor");
    }

    uint32_t maxRows() const { return max_rows_; }

private:
    MWHipWorldWrite(mwhip_exec *exec, uint64_t write, uint32_t max_rows, int32_t gpu_id)
        : ExecObject(exec, write, gpu_id), max_rows_(max_rows)
    {}

    uint32_t max_rows_;

friend class MWCudaExecutor;
};

// One number per world, element and term about one table, on the device:
// sums, minima, maxima, largest magnitudes, counts of non-zero and of
// non-finite values of chosen elements of chosen components over each world's
// rows in table order, each world's row count, and an alarm word per world
// that is 1 when a term flagged MWHIP_REDUCE_ALARM trips (mwhip_reduce_*,
// include/mwhip.h: the exact definition, the float sum's order included).
// compute() runs one kernel where the table is, sorted or not, and rewrites
// every tensor in full.  An extension of this backend.  Belongs to the
// executor that made it and must not outlive it.
class MWHipWorldReduce : public detail::ExecObject<detail::WorldReduceKind> {
public:
    MWHipWorldReduce() : num_terms_(0), is_float_ {} {}

    // waits for the executor's stream
    void compute() { req(mwhip_reduce_compute(exec_, handle_), "compute"); }
    // queued on the executor's stream behind the replays queued so far
    void computeAsync() { req(mwhip_reduce_compute_async(exec_, handle_), "computeAsync"); }

    // [worlds][num_elems] of term `term` (position in the list given to
    // makeWorldReduce) in the result type: Float32 for SUM / MIN / MAX of F32
    // and for ABSMAX, Int32 otherwise (py::Tensor has no unsigned 32-bit type:
    // the u32 results of U32 and U8 terms are those bits)
    py::Tensor termTensor(uint32_t term) const
    {
        uint64_t bytes = 0;
        uint32_t elems = 0;
        void *ptr = mwhip_reduce_buffer(exec_, handle_, term, &bytes, &elems);
        return tensor(ptr, is_float_[term] ? Elem::Float32 : Elem::Int32,
                      { numWorlds(), elems }, "termTensor");
    }

    // int32 [worlds]: each world's rows in the table
    py::Tensor countsTensor() const
    {
        return tensor(mwhip_reduce_counts(exec_, handle_), Elem::Int32,
                      { numWorlds() }, "countsTensor");
    }

    // int32 [worlds]: 1 where an alarm term tripped, else 0
    py::Tensor alarmTensor() const
    {
        return tensor(mwhip_reduce_alarm(exec_, handle_), Elem::Int32,
                      { numWorlds() }, "alarmTensor");
    }

    uint32_t numTerms() const { return num_terms_; }

private:
    MWHipWorldReduce(mwhip_exec *exec, uint64_t reduce, const mwhip_reduce_term *terms,
                     uint32_t n, int32_t gpu_id)
        : ExecObject(exec, reduce, gpu_id), num_terms_(n), is_float_ {}
    {
        for (uint32_t i = 0; i < n && i < MWHIP_REDUCE_MAX_TERMS; i++) {
            is_float_[i] = terms[i].dtype == MWHIP_REDUCE_F32 &&
                terms[i].op <= MWHIP_REDUCE_ABSMAX;
        }
    }

    uint32_t num_terms_;
    bool is_float_[MWHIP_REDUCE_MAX_TERMS];

friend class MWCudaExecutor;
};

// The cells of the entities a run of N handles in device memory names: per
// listed component uint8 [N][cell bytes] on the device (zero where a handle
// names nothing or its table has no such column), plus int32 [N] archetype and
// world of each (-1 where it names nothing), written in full by one kernel that
// goes through the entity store as Context::get<T>(e) does but trusts no bit
// of a handle (mwhip_gather_*, include/mwhip.h: the exact definition and what
// a valid source is -- never a table column's own address; read a column of
// handles through a world view's slab).  An extension of this backend.
// Belongs to the executor that made it and must not outlive it, nor its source.
class MWHipEntityGather : public detail::ExecObject<detail::EntityGatherKind> {
public:
    MWHipEntityGather() : num_handles_(0) {}

    // waits for the executor's stream
    void compute() { req(mwhip_gather_compute(exec_, handle_), "compute"); }
    // queued on the executor's stream behind the replays queued so far
    void computeAsync() { req(mwhip_gather_compute_async(exec_, handle_), "computeAsync"); }

    // uint8 [numHandles()][cell bytes] of listed component `column` (position
    // in the list given to makeEntityGather), owned by the executor
    py::Tensor columnTensor(uint32_t column) const
    {
        uint64_t bytes = 0;
        uint32_t cell = 0;
        void *ptr = mwhip_gather_buffer(exec_, handle_, column, &bytes, &cell);
        return tensor(ptr, Elem::UInt8, { num_handles_, cell }, "columnTensor");
    }

    // int32 [numHandles()]: the archetype of the entity each handle names, -1: none
    py::Tensor archetypesTensor() const
    {
        return tensor(mwhip_gather_archetypes(exec_, handle_), Elem::Int32,
                      { num_handles_ }, "archetypesTensor");
    }

    // int32 [numHandles()]: the world that entity is in, -1: none
    py::Tensor worldsTensor() const
    {
        return tensor(mwhip_gather_worlds(exec_, handle_), Elem::Int32,
                      { num_handles_ }, "worldsTensor");
    }

    uint64_t numHandles() const { return num_handles_; }

private:
    MWHipEntityGather(mwhip_exec *exec, uint64_t gather, uint64_t num_handles, int32_t gpu_id)
        : ExecObject(exec, gather, gpu_id), num_handles_(num_handles)
    {}

    uint64_t num_handles_;

friend class MWCudaExecutor;
};

// N = F x R rays, F fans of R rays that share an origin and a world, cast
// through the worlds' broadphase BVHs (BVH::traceRay / traceRayShared) by one
// kernel of the simulator's code object: per ray int32 status (MWHIP_RAYS_HIT,
// _MISS, _SKIPPED, _BAD_WORLD, _BAD_RAY), float hit_t, an Entity and a normal,
// with the conventions of a lidar system's outputs (0, Entity::none(), zero on
// anything but a hit).  mwhip_rays_*, include/mwhip.h, is the exact definition:
// which inputs are owned buffers and which the caller's sources, and that a ray
// sees the tree as the last broadphase pass left it, spheres being transparent.
// Needs a simulator that sets up a broadphase.  An extension of this backend.
// Belongs to the executor that made it and must not outlive it, nor its sources.
class MWHipRayQuery : public detail::ExecObject<detail::RayQueryKind> {
public:
    MWHipRayQuery() : num_fans_(0), num_rays_(0) {}

    // waits for the executor's stream
    void compute() { req(mwhip_rays_compute(exec_, handle_), "compute"); }
    // queued on the executor's stream behind the replays queued so far
    void computeAsync() { req(mwhip_rays_compute_async(exec_, handle_), "computeAsync"); }

    // inputs the query owns: int32 [numFans()] (no world source, no
    // fans_per_world), float [numFans()][3] (no origin source), float
    // [numRays()][3], float [numRays()]
    py::Tensor worldsTensor() const
    {
        return tensor(buffer(MWHIP_RAYS_BUF_WORLD), Elem::Int32, { num_fans_ }, "worldsTensor");
    }
    py::Tensor originsTensor() const
    {
        return tensor(buffer(MWHIP_RAYS_BUF_ORIGIN), Elem::Float32,
                      { num_fans_, 3 }, "originsTensor");
    }
    py::Tensor directionsTensor() const
    {
        return tensor(buffer(MWHIP_RAYS_BUF_DIR), Elem::Float32,
                      { num_rays_, 3 }, "directionsTensor");
    }
    py::Tensor tMaxTensor() const
    {
        return tensor(buffer(MWHIP_RAYS_BUF_T_MAX), Elem::Float32, { num_rays_ }, "tMaxTensor");
    }

    // outputs: float [numRays()], int32 [numRays()][2] (gen, id), float
    // [numRays()][3], int32 [numRays()]
    py::Tensor hitTTensor() const
    {
        return tensor(buffer(MWHIP_RAYS_BUF_HIT_T), Elem::Float32, { num_rays_ }, "hitTTensor");
    }
    py::Tensor hitsTensor() const
    {
        return tensor(buffer(MWHIP_RAYS_BUF_HIT), Elem::Int32, { num_rays_, 2 }, "hitsTensor");
    }
    py::Tensor normalsTensor() const
    {
        return tensor(buffer(MWHIP_RAYS_BUF_NORMAL), Elem::Float32,
                      { num_rays_, 3 }, "normalsTensor");
    }
    py::Tensor statusTensor() const
    {
        return tensor(buffer(MWHIP_RAYS_BUF_STATUS), Elem::Int32, { num_rays_ }, "statusTensor");
    }

    // the hits as the source of an entity gather or scatter
    mwhip_gather_source handleSource() const
    {
        void *ptr = buffer(MWHIP_RAYS_BUF_HIT);
        req(ptr != nullptr ? 0 : -1, "handleSource");
        return mwhip_gather_source { ptr, num_rays_, 8u, 0u, 1u, 0u };
    }

    uint64_t numFans() const { return num_fans_; }
    uint64_t numRays() const { return num_rays_; }

private:
    MWHipRayQuery(mwhip_exec *exec, uint64_t rays, uint64_t num_fans, uint64_t num_rays,
                  int32_t gpu_id)
        : ExecObject(exec, rays, gpu_id), num_fans_(num_fans), num_rays_(num_rays)
    {}

    void *buffer(uint32_t which) const
    {
        return mwhip_rays_buffer(exec_, handle_, which, nullptr);
    }

    uint64_t num_fans_;
    uint64_t num_rays_;

friend class MWCudaExecutor;
};

// B = F x G boxes, F bundles of G boxes that share a world and a centre, tested
// through the worlds' broadphase BVHs by one kernel of the simulator's code
// object: per box int32 status (MWHIP_BOXES_OK, _SKIPPED, _BAD_WORLD, _BAD_BOX),
// int32 count (how many entities PhysicsSystem::findEntitiesWithinAABB reports,
// not capped) and the first maxHits() of them as Entity handles in report
// order, Entity::none() behind them.  mwhip_boxes_*, include/mwhip.h, is the
// exact definition: pMin = centre + lo, pMax = centre + hi; which inputs are
// owned buffers and which the caller's sources; that a box sees the tree as the
// last broadphase pass left it and the poses as they are now.  Needs a
// simulator that sets up a broadphase.  An extension of this backend.  Belongs
// to the executor that made it and must not outlive it, nor its sources.
class MWHipBoxQuery : public detail::ExecObject<detail::BoxQueryKind> {
public:
    MWHipBoxQuery() : num_bundles_(0), num_boxes_(0), max_hits_(0) {}

    // waits for the executor's stream
    void compute() { req(mwhip_boxes_compute(exec_, handle_), "compute"); }
    // queued on the executor's stream behind the replays queued so far
    void computeAsync() { req(mwhip_boxes_compute_async(exec_, handle_), "computeAsync"); }

    // inputs the query owns: int32 [numBundles()] (no world source, no
    // bundles_per_world), float [numBundles()][3] (no centre source), float
    // [numBoxes()][3] twice
    py::Tensor worldsTensor() const
    {
        return tensor(buffer(MWHIP_BOXES_BUF_WORLD), Elem::Int32, { num_bundles_ }, "worldsTensor");
    }
    py::Tensor centresTensor() const
    {
        return tensor(buffer(MWHIP_BOXES_BUF_CENTRE), Elem::Float32,
                      { num_bundles_, 3 }, "centresTensor");
    }
    py::Tensor loTensor() const
    {
        return tensor(buffer(MWHIP_BOXES_BUF_LO), Elem::Float32, { num_boxes_, 3 }, "loTensor");
    }
    py::Tensor hiTensor() const
    {
        return tensor(buffer(MWHIP_BOXES_BUF_HI), Elem::Float32, { num_boxes_, 3 }, "hiTensor");
    }

    // outputs: int32 [numBoxes()] twice, int32 [numBoxes()][maxHits()][2]
    // (gen, id)
    py::Tensor statusTensor() const
    {
        return tensor(buffer(MWHIP_BOXES_BUF_STATUS), Elem::Int32, { num_boxes_ }, "statusTensor");
    }
    py::Tensor countsTensor() const
    {
        return tensor(buffer(MWHIP_BOXES_BUF_COUNT), Elem::Int32, { num_boxes_ }, "countsTensor");
    }
    py::Tensor hitsTensor() const
    {
        return tensor(buffer(MWHIP_BOXES_BUF_HITS), Elem::Int32,
                      { num_boxes_, max_hits_, 2 }, "hitsTensor");
    }

    // the hits as the source of an entity gather or scatter: numBoxes() x
    // maxHits() handles
    mwhip_gather_source handleSource() const
    {
        void *ptr = buffer(MWHIP_BOXES_BUF_HITS);
        req(ptr != nullptr ? 0 : -1, "handleSource");
        return mwhip_gather_source { ptr, num_boxes_ * max_hits_, 8u, 0u, 1u, 0u };
    }

    uint64_t numBundles() const { return num_bundles_; }
    uint64_t numBoxes() const { return num_boxes_; }
    uint64_t maxHits() const { return max_hits_; }

private:
    MWHipBoxQuery(mwhip_exec *exec, uint64_t boxes, uint64_t num_bundles, uint64_t num_boxes,
                  uint64_t max_hits, int32_t gpu_id)
        : ExecObject(exec, boxes, gpu_id), num_bundles_(num_bundles), num_boxes_(num_boxes),
          max_hits_(max_hits)
    {}

    void *buffer(uint32_t which) const
    {
        return mwhip_boxes_buffer(exec_, handle_, which, nullptr);
    }

    uint64_t num_bundles_;
    uint64_t num_boxes_;
    uint64_t max_hits_;

friend class MWCudaExecutor;
};

// Which bodies touch, where and how deep: per world int32 status
// (MWHIP_CONTACTS_OK, _SKIPPED, _UNSORTED, _UNSUPPORTED), int32 count (not capped)
// and the first maxContacts() contacts in the order (k_lo, k_hi, primitive
// pair) -- the Entity handles of the body that owns the reference feature and of
// the other, the number of points, the normal, and four points (xyz world
// position, w depth; zero from the number of points on).  mwhip_contacts_*,
// include/mwhip.h, is the exact definition: which pairs are tested, that solver
// poses (xpbd::PreSolvePositional) are the default and what
// MWHIP_CONTACTS_CURRENT_POSES takes instead, that no BVH is walked.  Needs a
// simulator that sets up a rigid-body step.  An extension of this backend.
// Belongs to the executor that made it and must not outlive it, nor its source.
class MWHipContactQuery : public detail::ExecObject<detail::ContactQueryKind> {
public:
    MWHipContactQuery() : num_worlds_(0), max_contacts_(0) {}

    // waits for the executor's stream
    void compute() { req(mwhip_contacts_compute(exec_, handle_), "compute"); }
    // queued on the executor's stream behind the replays queued so far
    void computeAsync() { req(mwhip_contacts_compute_async(exec_, handle_), "computeAsync"); }

    // the input the query owns if desc.own_select was set: int32 [numWorlds()]
    py::Tensor selectTensor() const
    {
        return tensor(buffer(MWHIP_CONTACTS_BUF_SELECT), Elem::Int32, { num_worlds_ },
                      "selectTensor");
    }

    // outputs: int32 [numWorlds()] twice; int32 [numWorlds()][maxContacts()][4]
    // (ref gen, ref id, alt gen, alt id); int32 [numWorlds()][maxContacts()];
    // float [numWorlds()][maxContacts()][3]; float [numWorlds()][maxContacts()][16]
    py::Tensor statusTensor() const
    {
        return tensor(buffer(MWHIP_CONTACTS_BUF_STATUS), Elem::Int32, { num_worlds_ },
                      "statusTensor");
    }
    py::Tensor countsTensor() const
    {
        return tensor(buffer(MWHIP_CONTACTS_BUF_COUNT), Elem::Int32, { num_worlds_ },
                      "countsTensor");
    }
    py::Tensor pairsTensor() const
    {
        return tensor(buffer(MWHIP_CONTACTS_BUF_PAIRS), Elem::Int32,
                      { num_worlds_, max_contacts_, 4 }, "pairsTensor");
    }
    py::Tensor numPointsTensor() const
    {
        return tensor(buffer(MWHIP_CONTACTS_BUF_NUM_POINTS), Elem::Int32,
                      { num_worlds_, max_contacts_ }, "numPointsTensor");
    }
    py::Tensor normalsTensor() const
    {
        return tensor(buffer(MWHIP_CONTACTS_BUF_NORMAL), Elem::Float32,
                      { num_worlds_, max_contacts_, 3 }, "normalsTensor");
    }
    py::Tensor pointsTensor() const
    {
        return tensor(buffer(MWHIP_CONTACTS_BUF_POINTS), Elem::Float32,
                      { num_worlds_, max_contacts_, 16 }, "pointsTensor");
    }

    // the pairs as the source of an entity gather or scatter: numWorlds() x
    // maxContacts() x 2 handles (a contact's ref, then its alt)
    mwhip_gather_source handleSource() const
    {
        void *ptr = buffer(MWHIP_CONTACTS_BUF_PAIRS);
        req(ptr != nullptr ? 0 : -1, "handleSource");
        return mwhip_gather_source { ptr, num_worlds_ * max_contacts_ * 2u, 8u, 0u, 1u, 0u };
    }

    uint64_t maxContacts() const { return max_contacts_; }

private:
    MWHipContactQuery(mwhip_exec *exec, uint64_t contacts, uint64_t num_worlds,
                      uint64_t max_contacts, int32_t gpu_id)
        : ExecObject(exec, contacts, gpu_id), num_worlds_(num_worlds),
          max_contacts_(max_contacts)
    {}

    void *buffer(uint32_t which) const
    {
        return mwhip_contacts_buffer(exec_, handle_, which, nullptr);
    }

    uint64_t num_worlds_;
    uint64_t max_contacts_;

friend class MWCudaExecutor;
};

// "If this object stood THERE, what would it touch, where, and how deep?":
// numShapes() = numBundles() x shapes-per-bundle posed collision shapes, the
// shapes of a bundle in one world, each tested against the rigid bodies of its
// world with the step's narrowphase.  Per shape int32 status (MWHIP_SHAPES_OK,
// _SKIPPED, _BAD_WORLD, _BAD_SHAPE, _UNSORTED, _UNSUPPORTED), int32 count (not
// capped) and the first maxHits() hits in the order (body, primitive pair): the
// Entity of the body touched, whether the contact's reference side is the
// shape, the number of points, the normal, and four points (xyz world position,
// w depth; zero from the number of points on).  mwhip_shapes_*, include/mwhip.h,
// is the exact definition: which pairs are tested, at the bodies' current
// poses, that no BVH is walked.  Needs a simulator that sets up a rigid-body
// step.  An extension of this backend.  Belongs to the executor that made it
// and must not outlive it, nor its sources.
class MWHipShapeQuery : public detail::ExecObject<detail::ShapeQueryKind> {
public:
    MWHipShapeQuery() : num_bundles_(0), num_shapes_(0), max_hits_(0) {}

    // waits for the executor's stream
    void compute() { req(mwhip_shapes_compute(exec_, handle_), "compute"); }
    // queued on the executor's stream behind the replays queued so far
    void computeAsync() { req(mwhip_shapes_compute_async(exec_, handle_), "computeAsync"); }

    // inputs the query owns: int32 [numBundles()] (no world source, no
    // bundles_per_world), int32 [numShapes()][2] (gen, id; no exclude source),
    // int32 [numShapes()], float [numShapes()][3], [numShapes()][4] (w, x, y, z)
    // and [numShapes()][3]
    py::Tensor worldsTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_WORLD), Elem::Int32, { num_bundles_ },
                      "worldsTensor");
    }
    py::Tensor excludesTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_EXCLUDE), Elem::Int32, { num_shapes_, 2 },
                      "excludesTensor");
    }
    py::Tensor objectsTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_OBJECT), Elem::Int32, { num_shapes_ },
                      "objectsTensor");
    }
    py::Tensor positionsTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_POSITION), Elem::Float32, { num_shapes_, 3 },
                      "positionsTensor");
    }
    py::Tensor rotationsTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_ROTATION), Elem::Float32, { num_shapes_, 4 },
                      "rotationsTensor");
    }
    py::Tensor scalesTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_SCALE), Elem::Float32, { num_shapes_, 3 },
                      "scalesTensor");
    }

    // outputs: int32 [numShapes()] twice; int32 [numShapes()][maxHits()][2]
    // (gen, id); int32 [numShapes()][maxHits()] twice; float
    // [numShapes()][maxHits()][3]; float [numShapes()][maxHits()][16]
    py::Tensor statusTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_STATUS), Elem::Int32, { num_shapes_ },
                      "statusTensor");
    }
    py::Tensor countsTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_COUNT), Elem::Int32, { num_shapes_ },
                      "countsTensor");
    }
    py::Tensor hitsTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_HITS), Elem::Int32, { num_shapes_, max_hits_, 2 },
                      "hitsTensor");
    }
    py::Tensor shapeIsRefTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_SHAPE_IS_REF), Elem::Int32,
                      { num_shapes_, max_hits_ }, "shapeIsRefTensor");
    }
    py::Tensor numPointsTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_NUM_POINTS), Elem::Int32,
                      { num_shapes_, max_hits_ }, "numPointsTensor");
    }
    py::Tensor normalsTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_NORMAL), Elem::Float32,
                      { num_shapes_, max_hits_, 3 }, "normalsTensor");
    }
    py::Tensor pointsTensor() const
    {
        return tensor(buffer(MWHIP_SHAPES_BUF_POINTS), Elem::Float32,
                      { num_shapes_, max_hits_, 16 }, "pointsTensor");
    }

    // the hits as the source of an entity gather or scatter: numShapes() x
    // maxHits() handles
    mwhip_gather_source handleSource() const
    {
        void *ptr = buffer(MWHIP_SHAPES_BUF_HITS);
        req(ptr != nullptr ? 0 : -1, "handleSource");
        return mwhip_gather_source { ptr, num_shapes_ * max_hits_, 8u, 0u, 1u, 0u };
    }

    uint64_t numBundles() const { return num_bundles_; }
    uint64_t numShapes() const { return num_shapes_; }
    uint64_t maxHits() const { return max_hits_; }

private:
    MWHipShapeQuery(mwhip_exec *exec, uint64_t shapes, uint64_t num_bundles,
                    uint64_t num_shapes, uint64_t max_hits, int32_t gpu_id)
        : ExecObject(exec, shapes, gpu_id), num_bundles_(num_bundles), num_shapes_(num_shapes),
          max_hits_(max_hits)
    {}

    void *buffer(uint32_t which) const
    {
        return mwhip_shapes_buffer(exec_, handle_, which, nullptr);
    }

    uint64_t num_bundles_;
    uint64_t num_shapes_;
    uint64_t max_hits_;

friend class MWCudaExecutor;
};

// The batched ctx.get<T>(e) = v: per listed component uint8 [N][cell bytes] on
// the device and int32 [N] select, filled by the caller; apply() stores cell i
// into the entity handle i of the source names, where select[i] != 0, and among
// selected handles that name the same entity the highest index wins.  int32 [N]
// archetype and world (-1 where a handle names nothing) and written (1 where
// handle i's cells are the ones now in the table) are rewritten by every apply.
// The other direction of an MWHipEntityGather, with its source and its handle
// checks (mwhip_scatter_*, include/mwhip.h: the exact definition).  Entity and
// WorldID cannot be listed; no rows are created or destroyed.  An extension of
// this backend.  Belongs to the executor that made it and must not outlive it,
// nor its source.
class MWHipEntityScatter : public detail::ExecObject<detail::EntityScatterKind> {
public:
    MWHipEntityScatter() : num_handles_(0) {}

    // waits for the executor's stream
    void apply() { req(mwhip_scatter_apply(exec_, handle_), "apply"); }
    // queued on the executor's stream behind the replays queued so far
    void applyAsync() { req(mwhip_scatter_apply_async(exec_, handle_), "applyAsync"); }

    // uint8 [numHandles()][cell bytes] of listed component `column` (position
    // in the list given to makeEntityScatter), owned by the executor: the input
    py::Tensor columnTensor(uint32_t column) const
    {
        uint64_t bytes = 0;
        uint32_t cell = 0;
        void *ptr = mwhip_scatter_buffer(exec_, handle_, column, &bytes, &cell);
        return tensor(ptr, Elem::UInt8, { num_handles_, cell }, "columnTensor");
    }

    // int32 [numHandles()]: non-zero where handle i's cells are to be stored (input)
    py::Tensor selectTensor() const
    {
        return tensor(mwhip_scatter_select(exec_, handle_), Elem::Int32,
                      { num_handles_ }, "selectTensor");
    }

    // int32 [numHandles()]: the archetype of the entity each handle names, -1: none
    py::Tensor archetypesTensor() const
    {
        return tensor(mwhip_scatter_archetypes(exec_, handle_), Elem::Int32,
                      { num_handles_ }, "archetypesTensor");
    }

    // int32 [numHandles()]: the world that entity is in, -1: none
    py::Tensor worldsTensor() const
    {
        return tensor(mwhip_scatter_worlds(exec_, handle_), Elem::Int32,
                      { num_handles_ }, "worldsTensor");
    }

    // int32 [numHandles()]: 1 where the last apply stored handle i's cells
    py::Tensor writtenTensor() const
    {
        return tensor(mwhip_scatter_written(exec_, handle_), Elem::Int32,
                      { num_handles_ }, "writtenTensor");
    }

    uint64_t numHandles() const { return num_handles_; }

private:
    MWHipEntityScatter(mwhip_exec *exec, uint64_t scatter, uint64_t num_handles, int32_t gpu_id)
        : ExecObject(exec, scatter, gpu_id), num_handles_(num_handles)
    {}

    uint64_t num_handles_;

friend class MWCudaExecutor;
};

namespace detail {

// A renderer's MeshBVHData / MaterialData (host or device memory) as the
// triangle description the executor's C ABI takes: every leaf child of every
// node names `triSize` consecutive triangles, three de-indexed BVHVertex each
// (reference mesh_bvh.hpp:33-47, bvh_raycast.cpp:303-313).
struct ReferenceAssets {
    std::vector<float> vertices;            // 3 per triangle corner
    std::vector<float> uvs;
    std::vector<uint32_t> indices;          // 0, 1, 2, ... per object
    std::vector<uint32_t> vertexOffsets { 0u };
    std::vector<uint32_t> triangleOffsets { 0u };
    std::vector<int32_t> triangleMaterials;
    std::vector<int32_t> objectMaterials;
    std::vector<float> materialColors;
    std::vector<int32_t> materialTextures;
    std::vector<render::TextureRGBA8> textureDescs;

    template <typename T>
    static std::vector<T> fetch(const T *src, uint64_t count)
    {
        std::vector<T> host(count);
        if (count != 0 && mwhip_memcpy_any(host.data(), src,
                                           count * sizeof(T)) != 0) {
            fprintf(stderr, "madrona_amd: cannot read the render assets: %s\n",
                    mwhip_last_error());
            abort();
        }
        return host;
    }

    template <typename ConfigT>
    void read(const ConfigT &cfg)
    {
        const render::MeshBVHData &geo = cfg.geoBVHData;
        const std::vector<MeshBVH> meshes = fetch(geo.meshBVHs, geo.numBVHs);
        int32_t max_material = -1;
        for (const MeshBVH &mesh : meshes) {
            const std::vector<QBVHNode> nodes = fetch(mesh.nodes, mesh.numNodes);
            const std::vector<MeshBVH::BVHVertex> verts =
                fetch(mesh.vertices, mesh.numVerts);
            const std::vector<MeshBVH::LeafMaterial> leaf_mats =
                mesh.materialIDX == -1 && mesh.leafMats != nullptr ?
                    fetch(mesh.leafMats, mesh.numVerts / 3u) :
                    std::vector<MeshBVH::LeafMaterial>();
            uint32_t corner = 0;
            for (const QBVHNode &node : nodes) {
                for (uint32_t c = 0; c < (uint32_t)MADRONA_BVH_WIDTH; c++) {
                    if (!node.hasChild(c) || !node.isLeaf(c)) continue;
                    const uint32_t first = node.leafIDX(c);
                    for (uint32_t t = 0; t < node.triSize[c]; t++) {
                        for (uint32_t k = 0; k < 3u; k++) {
                            const MeshBVH::BVHVertex &v =
                                verts[(size_t)(first + t) * 3u + k];
                            vertices.insert(vertices.end(),
                                            { v.pos.x, v.pos.y, v.pos.z });
                            uvs.insert(uvs.end(), { v.uv.x, v.uv.y });
                            indices.push_back(corner++);
                        }
                        const int32_t m = leaf_mats.empty() ? -1 :
                            leaf_mats[first + t].material[0].matIDX;
                        triangleMaterials.push_back(m);
                        max_material = m > max_material ? m : max_material;
                    }
                }
            }
            vertexOffsets.push_back((uint32_t)(vertices.size() / 3));
            triangleOffsets.push_back((uint32_t)(indices.size() / 3));
            objectMaterials.push_back(mesh.materialIDX);
            max_material = mesh.materialIDX > max_material ?
                mesh.materialIDX : max_material;
        }

        const uint32_t num_materials = cfg.numMaterials != 0 ?
            cfg.numMaterials : (uint32_t)(max_material + 1);
        const std::vector<Material> materials =
            fetch(cfg.materialData.materials,
                  cfg.materialData.materials != nullptr ? num_materials : 0u);
        for (const Material &m : materials) {
            materialColors.insert(materialColors.end(),
                                  { m.color.x, m.color.y, m.color.z });
            materialTextures.push_back(m.textureIdx);
        }
        const std::vector<cudaTextureObject_t> handles = fetch(
            cfg.materialData.textures, cfg.materialData.numTextureBuffers);
        for (cudaTextureObject_t h : handles) {
            textureDescs.push_back(*(const render::TextureRGBA8 *)(uintptr_t)h);
        }
    }

    void describe(mwhip_render_geometry &geometry,
                  std::vector<mwhip_texture> &textures) const
    {
        geometry.num_objects = (uint32_t)triangleOffsets.size() - 1u;
        geometry.vertices = vertices.data();
        geometry.indices = indices.data();
        geometry.object_vertex_offset = vertexOffsets.data();
        geometry.object_triangle_offset = triangleOffsets.data();
        geometry.vertex_uv = uvs.data();
        geometry.triangle_material = triangleMaterials.data();
        geometry.object_material = objectMaterials.data();
        geometry.num_materials = (uint32_t)(materialColors.size() / 3);
        geometry.material_color = materialColors.data();
        if (!textureDescs.empty()) {
            geometry.material_texture = materialTextures.data();
            for (const render::TextureRGBA8 &t : textureDescs) {
                textures.push_back({ t.width, t.height, t.pixels });
            }
            geometry.num_textures = (uint32_t)textures.size();
            geometry.textures = textures.data();
        }
    }
};

}

class MWCudaExecutor {
    using ReferenceAssets = detail::ReferenceAssets;
public:
    static CUcontext initCUDA(int gpu_id) { return CUcontext { gpu_id }; }

    MWCudaExecutor() : exec_(nullptr), num_taskgraphs_(0), gpu_id_(0) {}

    MWCudaExecutor(const StateConfig &state_cfg,
                   const CompileConfig &,
                   CUcontext ctx,
                   Optional<CudaBatchRenderConfig> render_cfg =
                       Optional<CudaBatchRenderConfig>::none())
        : exec_(nullptr), num_taskgraphs_(state_cfg.numTaskGraphs), gpu_id_(ctx.gpuID)
    {
        mwhip_state_config cfg {};
        mwhip_render_geometry geometry {};
        std::vector<mwhip_texture> textures;
        ReferenceAssets from_reference;
        if (render_cfg.has_value()) {
            const render::TriangleMeshData &geo = render_cfg->geoTriangles;
            if (render_cfg->geoBVHData.numBVHs != 0) {
                // the reference's asset form: read the leaves of its mesh BVHs
                from_reference.read(*render_cfg);
                from_reference.describe(geometry, textures);
                cfg.render_geometry = &geometry;
            } else if (geo.objectTriangleOffsets.size() > 1) {
                geometry.num_objects =
                    (uint32_t)geo.objectTriangleOffsets.size() - 1u;
                geometry.vertices = (const float *)geo.vertices.data();
                geometry.indices = geo.indices.data();
                geometry.object_vertex_offset = geo.objectVertexOffsets.data();
                geometry.object_triangle_offset =
                    geo.objectTriangleOffsets.data();
                geometry.vertex_uv = geo.vertexUVs.size() != 0 ?
                    (const float *)geo.vertexUVs.data() : nullptr;
                geometry.triangle_material = geo.triangleMaterials.size() != 0 ?
                    geo.triangleMaterials.data() : nullptr;
                const render::TriangleMaterialData &mats =
                    render_cfg->triangleMaterials;
                geometry.num_materials = (uint32_t)mats.materialColors.size();
                geometry.material_color =
                    (const float *)mats.materialColors.data();
                geometry.object_material = mats.objectMaterials.size() != 0 ?
                    mats.objectMaterials.data() : nullptr;
                if (mats.materialTextures.size() != 0) {
                    geometry.material_texture = mats.materialTextures.data();
                    for (const render::TextureRGBA8 &t : mats.textures) {
                        textures.push_back({ t.width, t.height, t.pixels });
                    }
                    geometry.num_textures = (uint32_t)textures.size();
                    geometry.textures = textures.data();
                }
                cfg.render_geometry = &geometry;
            }
            cfg.raycast_output_resolution = render_cfg->renderResolution;
            cfg.raycast_max_views_per_world = render_cfg->maxViewsPerWorld;
            cfg.raycast_rgbd = render_cfg->renderMode ==
                CudaBatchRenderConfig::RenderMode::RGBD ? 1u : 0u;
            cfg.object_root_aabbs = render_cfg->objectRootAABBs.data();
            cfg.num_object_root_aabbs =
                (uint32_t)render_cfg->objectRootAABBs.size() / 6u;
        }
        cfg.world_init_ptr = state_cfg.worldInitPtr;
        cfg.num_world_init_bytes = state_cfg.numWorldInitBytes;
        cfg.user_config_ptr = state_cfg.userConfigPtr;
        cfg.num_user_config_bytes = state_cfg.numUserConfigBytes;
        cfg.num_world_data_bytes = state_cfg.numWorldDataBytes;
        cfg.world_data_alignment = state_cfg.worldDataAlignment;
        cfg.num_worlds = state_cfg.numWorlds;
        cfg.num_task_graphs = state_cfg.numTaskGraphs;
        cfg.num_exported_buffers = state_cfg.numExportedBuffers;
        cfg.gpu_id = ctx.gpuID;

        req(mwhip_create(&cfg, madronaMWHipUserEntry(), &exec_),
            "MWCudaExecutor");
    }

    MWCudaExecutor(const MWCudaExecutor &) = delete;
    MWCudaExecutor(MWCudaExecutor &&o)
        : exec_(o.exec_), num_taskgraphs_(o.num_taskgraphs_), gpu_id_(o.gpu_id_)
    {
        o.exec_ = nullptr;
    }

    ~MWCudaExecutor()
    {
        if (exec_ != nullptr) {
            mwhip_destroy(exec_);
        }
    }

    MWCudaExecutor &operator=(MWCudaExecutor &&o)
    {
        if (this != &o) {
            if (exec_ != nullptr) {
                mwhip_destroy(exec_);
            }
            exec_ = o.exec_;
            num_taskgraphs_ = o.num_taskgraphs_;
            gpu_id_ = o.gpu_id_;
            o.exec_ = nullptr;
        }
        return *this;
    }

    template <EnumType EnumT>
    MWCudaLaunchGraph buildLaunchGraph(EnumT taskgraph_id,
                                       const char *stat_name = nullptr)
    {
        return buildLaunchGraph((uint32_t)taskgraph_id, stat_name);
    }

    MWCudaLaunchGraph buildLaunchGraph(uint32_t taskgraph_id,
                                       const char *stat_name = nullptr)
    {
        return buildLaunchGraph(Span<const uint32_t>(&taskgraph_id, 1),
                                stat_name);
    }

    MWCudaLaunchGraph buildLaunchGraph(Span<const uint32_t> taskgraph_ids,
                                       const char *stat_name = nullptr)
    {
        uint64_t graph = 0;
        req(mwhip_build_launch_graph(exec_, taskgraph_ids.data(),
            (uint32_t)taskgraph_ids.size(), stat_name, &graph),
            "buildLaunchGraph");
        return MWCudaLaunchGraph(exec_, graph);
    }

    MWCudaLaunchGraph buildLaunchGraphAllTaskGraphs()
    {
        std::vector<uint32_t> ids(num_taskgraphs_);
        for (uint32_t i = 0; i < num_taskgraphs_; i++) ids[i] = i;
        return buildLaunchGraph(
            Span<const uint32_t>(ids.data(), (CountT)ids.size()));
    }

    // TLAS build + ray cast of every view into the RaycastOutputArchetype
    // columns (reference mw_gpu.hpp:150, cuda_exec.cpp:2527-2700); run it after
    // the step graph
    MWCudaLaunchGraph buildRenderGraph()
    {
        uint64_t graph = 0;
        req(mwhip_build_render_graph(exec_, &graph), "buildRenderGraph");
        return MWCudaLaunchGraph(exec_, graph);
    }

    // synchronous (reference cuda_exec.cpp:2756-2794)
    void run(MWCudaLaunchGraph &launch_graph)
    {
        req(mwhip_run(exec_, launch_graph.graph_), "run");
    }

    // strm is a hipStream_t
    void runAsync(MWCudaLaunchGraph &launch_graph, void *strm)
    {
        req(mwhip_run_async(exec_, launch_graph.graph_, strm), "runAsync");
    }

    // device pointer, owned by the executor
    void *getExported(CountT slot) const
    {
        return mwhip_get_exported(exec_, (uint32_t)slot);
    }

    // an empty snapshot of this executor's worlds (see MWHipSnapshot)
    MWHipSnapshot makeSnapshot()
    {
        uint64_t snapshot = 0;
        req(mwhip_snapshot_create(exec_, &snapshot), "makeSnapshot");
        return MWHipSnapshot(exec_, snapshot, gpu_id_);
    }

    // a digest of the listed columns of this executor's worlds (see MWHipDigest)
    MWHipDigest makeDigest(Span<const DigestColumn> columns)
    {
        uint64_t digest = 0;
        req(mwhip_digest_create(exec_, (const mwhip_digest_column *)columns.data(),
            (uint32_t)columns.size(), &digest), "makeDigest");
        return MWHipDigest(exec_, digest, gpu_id_);
    }

    // every replay of a step graph recomputes `digest` behind its task-graph
    // nodes and before its pack node and output rings; nullptr: none
    void setStepDigest(const MWHipDigest *digest)
    {
        setStep(mwhip_set_step_digest, digest, "setStepDigest");
    }

    // a padded per-world view of `components` of archetype `archetype`'s table,
    // max_rows rows per world (see MWHipWorldView)
    MWHipWorldView makeWorldView(uint32_t archetype, Span<const uint32_t> components,
                                 uint32_t max_rows)
    {
        uint64_t view = 0;
        req(mwhip_view_create(exec_, archetype, components.data(),
            (uint32_t)components.size(), max_rows, &view), "makeWorldView");
        return MWHipWorldView(exec_, view, max_rows, gpu_id_);
    }

    // on: every replay of a step graph recomputes `view` behind its task-graph
    // nodes and before its pack node and output rings (up to
    // MWHIP_MAX_STEP_VIEWS views, one launch for all); off: no longer
    void setStepView(const MWHipWorldView *view, bool on)
    {
        setStep(mwhip_set_step_view, view, "setStepView", on ? 1 : 0);
    }

    // tensors to scatter into `components` of archetype `archetype`'s table
    // (neither Entity nor WorldID), max_rows rows per world (see MWHipWorldWrite)
    MWHipWorldWrite makeWorldWrite(uint32_t archetype, Span<const uint32_t> components,
                                   uint32_t max_rows)
    {
        uint64_t write = 0;
        req(mwhip_write_create(exec_, archetype, components.data(),
            (uint32_t)components.size(), max_rows, &write), "makeWorldWrite");
        return MWHipWorldWrite(exec_, write, max_rows, gpu_id_);
    }

    // on: every replay of a step graph applies `write` behind its input rings
    // and in front of its first task-graph node (up to MWHIP_MAX_STEP_WRITES
    // writes, one launch for all); off: no longer
    void setStepWrite(const MWHipWorldWrite *write, bool on)
    {
        setStep(mwhip_set_step_write, write, "setStepWrite", on ? 1 : 0);
    }

    // per-world reductions of archetype `archetype`'s table, one per term (see
    // MWHipWorldReduce and mwhip_reduce_term)
    MWHipWorldReduce makeWorldReduce(uint32_t archetype, const mwhip_reduce_term *terms,
                                     uint32_t n)
    {
        uint64_t reduce = 0;
        req(mwhip_reduce_create(exec_, archetype, terms, n, &reduce), "makeWorldReduce");
        return MWHipWorldReduce(exec_, reduce, terms, n, gpu_id_);
    }

    // on: every replay of a step graph recomputes `reduce` behind its step
    // views and in front of its pack node and output rings (up to
    // MWHIP_MAX_STEP_REDUCES reduces, one launch for all); off: no longer
    void setStepReduce(const MWHipWorldReduce *reduce, bool on)
    {
        setStep(mwhip_set_step_reduce, reduce, "setStepReduce", on ? 1 : 0);
    }

    // the cells of `components` (component ids) of the entities the handles of
    // `source` name (see MWHipEntityGather and mwhip_gather_source)
    MWHipEntityGather makeEntityGather(const mwhip_gather_source &source,
                                       Span<const uint32_t> components)
    {
        uint64_t gather = 0;
        req(mwhip_gather_create(exec_, &source, components.data(),
            (uint32_t)components.size(), &gather), "makeEntityGather");
        return MWHipEntityGather(exec_, gather,
                                 source.num_records * source.handles_per_record, gpu_id_);
    }

    // on: every replay of a step graph recomputes `gather` directly behind its
    // step views, whose slabs it may read, and in front of its pack node and
    // output rings (up to MWHIP_MAX_STEP_GATHERS gathers, one launch for all);
    // off: no longer
    void setStepGather(const MWHipEntityGather *gather, bool on)
    {
        setStep(mwhip_set_step_gather, gather, "setStepGather", on ? 1 : 0);
    }

    // cells of `components` (component ids; neither Entity nor WorldID) written
    // into the entities the handles of `source` name (see MWHipEntityScatter)
    MWHipEntityScatter makeEntityScatter(const mwhip_gather_source &source,
                                         Span<const uint32_t> components)
    {
        uint64_t scatter = 0;
        req(mwhip_scatter_create(exec_, &source, components.data(),
            (uint32_t)components.size(), &scatter), "makeEntityScatter");
        return MWHipEntityScatter(exec_, scatter,
                                  source.num_records * source.handles_per_record, gpu_id_);
    }

    // on: every replay of a step graph applies `scatter` directly behind its
    // step writes (on the same cell the scatter wins) and in front of its first
    // node (up to MWHIP_MAX_STEP_SCATTERS scatters that list disjoint
    // components, three launches for all); off: no longer
    void setStepScatter(const MWHipEntityScatter *scatter, bool on)
    {
        setStep(mwhip_set_step_scatter, scatter, "setStepScatter", on ? 1 : 0);
    }

    // desc.num_fans fans of desc.rays_per_fan rays through the worlds'
    // broadphase BVHs (see MWHipRayQuery and mwhip_rays_desc)
    MWHipRayQuery makeRayQuery(const mwhip_rays_desc &desc)
    {
        uint64_t rays = 0;
        req(mwhip_rays_create(exec_, &desc, &rays), "makeRayQuery");
        return MWHipRayQuery(exec_, rays, desc.num_fans,
                             (uint64_t)desc.num_fans * desc.rays_per_fan, gpu_id_);
    }

    // on: every replay of a step graph recomputes `rays` behind its step views
    // (whose slabs and counts it may read) and in front of its step gathers
    // (which may read the hits), its pack node and its output rings (up to
    // MWHIP_MAX_STEP_RAYS queries, one launch for all); off: no longer
    void setStepRays(const MWHipRayQuery *rays, bool on)
    {
        setStep(mwhip_set_step_rays, rays, "setStepRays", on ? 1 : 0);
    }

    // desc.num_bundles bundles of desc.boxes_per_bundle boxes through the
    // worlds' broadphase BVHs, up to desc.max_hits entities listed per box (see
    // MWHipBoxQuery and mwhip_boxes_desc)
    MWHipBoxQuery makeBoxQuery(const mwhip_boxes_desc &desc)
    {
        uint64_t boxes = 0;
        req(mwhip_boxes_create(exec_, &desc, &boxes), "makeBoxQuery");
        return MWHipBoxQuery(exec_, boxes, desc.num_bundles,
                             (uint64_t)desc.num_bundles * desc.boxes_per_bundle, desc.max_hits,
                             gpu_id_);
    }

    // on: every replay of a step graph recomputes `boxes` directly behind its
    // step ray queries (hence behind its step views, whose slabs and counts it
    // may read) and in front of its step gathers (which may read the hits), its
    // pack node and its output rings (up to MWHIP_MAX_STEP_BOXES queries, one
    // launch for all); off: no longer
    void setStepBoxes(const MWHipBoxQuery *boxes, bool on)
    {
        setStep(mwhip_set_step_boxes, boxes, "setStepBoxes", on ? 1 : 0);
    }

    // per world up to desc.max_contacts touching primitive pairs of its rigid
    // bodies with their manifolds (see MWHipContactQuery and
    // mwhip_contacts_desc)
    MWHipContactQuery makeContactQuery(const mwhip_contacts_desc &desc)
    {
        uint64_t contacts = 0;
        req(mwhip_contacts_create(exec_, &desc, &contacts), "makeContactQuery");
        return MWHipContactQuery(exec_, contacts, mwhip_num_worlds(exec_), desc.max_contacts,
                                 gpu_id_);
    }

    // on: every replay of a step graph recomputes `contacts` directly behind
    // its step box queries and in front of its step gathers (which may read
    // the pairs), its pack node and its output rings (up to
    // MWHIP_MAX_STEP_CONTACTS queries, one launch for all); off: no longer
    void setStepContacts(const MWHipContactQuery *contacts, bool on)
    {
        setStep(mwhip_set_step_contacts, contacts, "setStepContacts", on ? 1 : 0);
    }

    // desc.num_bundles x desc.shapes_per_bundle posed collision shapes tested
    // against the bodies of their worlds, up to desc.max_hits hits each with
    // their manifolds (see MWHipShapeQuery and mwhip_shapes_desc)
    MWHipShapeQuery makeShapeQuery(const mwhip_shapes_desc &desc)
    {
        uint64_t shapes = 0;
        req(mwhip_shapes_create(exec_, &desc, &shapes), "makeShapeQuery");
        return MWHipShapeQuery(exec_, shapes, desc.num_bundles,
                               (uint64_t)desc.num_bundles * desc.shapes_per_bundle,
                               desc.max_hits, gpu_id_);
    }

    // on: every replay of a step graph recomputes `shapes` directly behind its
    // step contact queries and in front of its step gathers (which may read
    // the hits), its pack node and its output rings (up to
    // MWHIP_MAX_STEP_SHAPES queries, one launch for all); off: no longer
    void setStepShapes(const MWHipShapeQuery *shapes, bool on)
    {
        setStep(mwhip_set_step_shapes, shapes, "setStepShapes", on ? 1 : 0);
    }

    // Device-resident rings (extensions of this backend, include/mwhip.h).
    // The k-th replay of a step graph after the call starts by copying slot
    // k % num_slots of `ring` (whole dwords) into `dst`, normally an exported
    // action column; ring == nullptr removes the ring of dst
    void setInputRing(void *dst, const void *ring, uint64_t slot_bytes,
                      uint32_t num_slots)
    {
        req(mwhip_set_input_ring(exec_, dst, ring, slot_bytes, num_slots),
            "setInputRing");
    }

    // ... and ends (before its health kernel) by copying slot_bytes bytes of
    // `src` into slot k % num_slots of `ring`; on_render: replays of a render
    // graph record instead.  ring == nullptr removes the ring of (src, kind)
    void setOutputRing(const void *src, void *ring, uint64_t slot_bytes,
                       uint32_t num_slots, bool on_render = false)
    {
        req(mwhip_set_output_ring(exec_, src, ring, slot_bytes, num_slots,
                on_render ? MWHIP_RING_ON_RENDER : MWHIP_RING_ON_STEP),
            "setOutputRing");
    }

    // replays that have recorded into that ring since it was set (waits for
    // the executor's stream; not modulo its slots)
    uint64_t outputRingRecorded(const void *src, bool on_render = false)
    {
        uint64_t replays = 0;
        req(mwhip_output_ring_recorded(exec_, src,
                on_render ? MWHIP_RING_ON_RENDER : MWHIP_RING_ON_STEP, &replays),
            "outputRingRecorded");
        return replays;
    }

    mwhip_exec *handle() const { return exec_; }

private:
    static void req(int rc, const char *what)
    {
        if (rc != 0) {
            fprintf(stderr, "madrona_amd: %s failed (%d): %s\n", what, rc,
                    mwhip_last_error());
            abort();
        }
    }

    // mwhip_set_step_<kind>(exec, the handle of obj or 0, on...): the digest's
    // takes no `on`
    template <typename Obj, typename... On>
    void setStep(int (*set)(mwhip_exec *, uint64_t, On...), const Obj *obj, const char *what,
                 On... on)
    {
        req(set(exec_, obj != nullptr ? obj->handle() : 0, on...), what);
    }

    mwhip_exec *exec_;
    uint32_t num_taskgraphs_;
    int32_t gpu_id_;
};

using MWHipExecutor = MWCudaExecutor;
using MWHipLaunchGraph = MWCudaLaunchGraph;

}
