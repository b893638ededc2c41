#include "mesh_cast/sim.hpp"
#include "mesh_cast/meshes.hpp"

#ifndef SIM_BACKEND_REF_CPU
#include <madrona/mesh_bvh_upload.hpp>
#endif

struct SimTraits;
#include "common/sim_c_api.h"

#include <cstring>
#include <mutex>
#include <vector>
#include <string>

namespace simmgr { struct TensorDesc; struct ColumnList; }

namespace mesh_cast {

// The MeshBVH array worlds index (Sim::Config::meshes): the host trees on the
// reference CPU backend; on the HIP backend each tree uploaded
// (uploadMeshBVH) and the array of the uploaded structs uploaded in turn.
// Built once per process and device under a lock, never freed: simulators of
// one process share it.
static madrona::MeshBVH *configMeshes(int gpu_id)
{
    FamilyTrees &trees = familyTrees();
#ifdef SIM_BACKEND_REF_CPU
    (void)gpu_id;
    return trees.bvh;
#else
    static std::mutex lock;
    static std::vector<std::pair<int, madrona::MeshBVH *>> uploaded;
    std::lock_guard<std::mutex> guard(lock);
    for (auto &[id, ptr] : uploaded) {
        if (id == gpu_id) {
            return ptr;
        }
    }

    madrona::MeshBVH dev[kNumWorldFamilies];
    for (uint32_t f = 0; f < kNumWorldFamilies; f++) {
        dev[f] = madrona::uploadMeshBVH(gpu_id, trees.bvh[f]);
        if (dev[f].nodes == nullptr) {
            fprintf(stderr, "mesh_cast: uploading mesh %u failed\n", f);
            abort();
        }
    }
    auto *dev_array = (madrona::MeshBVH *)mwhip_raw_alloc(gpu_id, sizeof(dev));
    if (dev_array == nullptr ||
            mwhip_raw_copy_h2d(gpu_id, dev_array, dev, sizeof(dev)) != 0) {
        fprintf(stderr, "mesh_cast: uploading the mesh array failed\n");
        abort();
    }
    uploaded.push_back({ gpu_id, dev_array });
    return dev_array;
#endif
}

}

struct SimTraits {
    using Sim = mesh_cast::Sim;
    using Engine = mesh_cast::Engine;

    static constexpr uint32_t numExports =
        (uint32_t)mesh_cast::ExportID::NumExports;
    static constexpr uint32_t numTaskGraphs = 1;

    static Sim::Config makeConfig(const SimCreateArgs &args)
    {
        return Sim::Config { args.seed, args.world_base,
                             mesh_cast::configMeshes(args.gpu_id),
                             mesh_cast::kNumWorldFamilies };
    }

    static void makeInits(const SimCreateArgs &, Sim::WorldInit *) {}

    template <typename T>
    static void describeTensors(T &out, uint32_t num_worlds);
    template <typename T>
    static void describeColumns(T &cols);
};

#include "common/mgr_impl.inl"

template <typename T>
void SimTraits::describeTensors(T &out, uint32_t num_worlds)
{
    using mesh_cast::ExportID;
    int64_t W = num_worlds;
    int64_t A = mesh_cast::kAgentsPerWorld;
    out.push_back({ "position", SIM_F32, { W, A, 4 }, (uint32_t)ExportID::Position });
    out.push_back({ "sweep", SIM_F32, { W, A, 4 }, (uint32_t)ExportID::Sweep });
    // count, then the fp32 sum: raw 32-bit words
    out.push_back({ "overlap", SIM_I32, { W, A, 4 }, (uint32_t)ExportID::Overlap });
    out.push_back({ "ray_t", SIM_I32, { W, A, mesh_cast::kNumRays }, (uint32_t)ExportID::RayT });
}

template <typename T>
void SimTraits::describeColumns(T &cols)
{
    using namespace mesh_cast;
    cols.template add<Agent, madrona::Entity>("Agent.Entity", false);
    cols.template add<Agent, AgentPos>("Agent.AgentPos", false);
    cols.template add<Agent, RayT>("Agent.RayT", false);
    cols.template add<Agent, RayMaterial>("Agent.RayMaterial", false);
    cols.template add<Agent, RayNormal>("Agent.RayNormal", false);
    cols.template add<Agent, RayUV>("Agent.RayUV", false);
    cols.template add<Agent, SweepResult>("Agent.SweepResult", false);
    cols.template add<Agent, OverlapResult>("Agent.OverlapResult", false);
    cols.template add<Agent, AgentInfo>("Agent.AgentInfo", false);
}

// ---------------------------------------------------------------------------
// Host probes: each MeshBVH query over mesh family `family` for a caller's
// batch, and the built trees themselves.  In the reference-CPU build of this
// file these run the reference's mesh_bvh.inl, in the HIP build the header
// overlay's host path: the tests diff one against the other.

using madrona::MeshBVH;
using madrona::QBVHNode;
using madrona::math::Vector3;
using madrona::math::AABB;

static MeshBVH *probeTree(uint32_t family)
{
    if (family >= mesh_cast::kNumFamilies) {
        return nullptr;
    }
    return &mesh_cast::familyTrees().bvh[family];
}

extern "C" {

SIM_API uint32_t mesh_cast_num_families() { return mesh_cast::kNumFamilies; }

// counts: { nodes, leaves, numVerts, vertices in the array with the padded
// tail, source triangles }; root_aabb: pMin, pMax
SIM_API int32_t mesh_cast_tree_info(uint32_t family, uint32_t *counts,
                                    float *root_aabb)
{
    MeshBVH *bvh = probeTree(family);
    if (bvh == nullptr || bvh->nodes == nullptr) return -1;
    counts[0] = bvh->numNodes;
    counts[1] = bvh->numLeaves;
    counts[2] = bvh->numVerts;
    counts[3] = bvh->numVerts + 3 * (uint32_t)(MeshBVH::numTrisPerLeaf - 1);
    counts[4] = mesh_cast::familyTrees().data[family].numTris();
    memcpy(root_aabb, &bvh->rootAABB, sizeof(float) * 6);
    return bvh->materialIDX;
}

// nodes: 60 bytes each; materials: one per triangle; vertices: x y z u v each,
// padded tail included
SIM_API void mesh_cast_tree_arrays(uint32_t family, void *nodes,
                                   int32_t *materials, float *vertices)
{
    MeshBVH *bvh = probeTree(family);
    memcpy(nodes, bvh->nodes, sizeof(QBVHNode) * bvh->numNodes);
    memcpy(materials, bvh->leafMats,
           sizeof(MeshBVH::LeafMaterial) * (bvh->numVerts / 3));
    memcpy(vertices, bvh->vertices, sizeof(MeshBVH::BVHVertex) *
        (bvh->numVerts + 3 * (uint32_t)(MeshBVH::numTrisPerLeaf - 1)));
}

// the family's source triangles: 9 floats (3 positions), 6 floats (3 uvs) and
// a material each, in input order
SIM_API void mesh_cast_source_tris(uint32_t family, float *positions,
                                   float *uvs, int32_t *materials)
{
    const mesh_cast::MeshData &m = mesh_cast::familyTrees().data[family];
    for (uint32_t t = 0; t < m.numTris(); t++) {
        for (uint32_t c = 0; c < 3; c++) {
            uint32_t v = m.indices[3 * t + c];
            memcpy(positions + 9 * t + 3 * c, &m.positions[v],
                   sizeof(float) * 3);
            uvs[6 * t + 2 * c] = m.uvs.empty() ? 0.f : m.uvs[v].x;
            uvs[6 * t + 2 * c + 1] = m.uvs.empty() ? 0.f : m.uvs[v].y;
        }
        materials[t] = (int32_t)(m.faceMaterials.empty() ? m.materialIDX :
                                 m.faceMaterials[t]);
    }
}

// per ray: origins / dirs xyz, t_max; out: hit flag, tHit, normal xyz, uv,
// leafMaterialIDX, getMaterialIDX (zeros where the ray misses)
SIM_API void mesh_cast_trace(uint32_t family, uint32_t n,
                             const float *origins, const float *dirs,
                             const float *t_max, uint32_t *hit, float *t_hit,
                             float *normals, float *uvs, uint32_t *leaf_mat,
                             uint32_t *material)
{
    MeshBVH *bvh = probeTree(family);
    for (uint32_t i = 0; i < n; i++) {
        int32_t stack[32];
        int32_t stack_size = 0;
        MeshBVH::HitInfo info {};
        bool h = bvh->traceRay(
            Vector3 { origins[3 * i], origins[3 * i + 1], origins[3 * i + 2] },
            Vector3 { dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2] },
            &info, stack, stack_size, t_max[i]);
        hit[i] = h ? 1u : 0u;
        t_hit[i] = h ? info.tHit : 0.f;
        normals[3 * i] = h ? info.normal.x : 0.f;
        normals[3 * i + 1] = h ? info.normal.y : 0.f;
        normals[3 * i + 2] = h ? info.normal.z : 0.f;
        uvs[2 * i] = h ? info.uv.x : 0.f;
        uvs[2 * i + 1] = h ? info.uv.y : 0.f;
        leaf_mat[i] = h ? info.leafMaterialIDX : 0u;
        material[i] = h ? bvh->getMaterialIDX(info) : 0u;
    }
}

// per sweep: origin, move, radius, t_max; out: t, normal (zero where t == t_max)
SIM_API void mesh_cast_sweep(uint32_t family, uint32_t n,
                             const float *origins, const float *dirs,
                             const float *radii, const float *t_max,
                             float *t_out, float *normals)
{
    MeshBVH *bvh = probeTree(family);
    for (uint32_t i = 0; i < n; i++) {
        Vector3 normal { 0.f, 0.f, 0.f };
        float t = bvh->sphereCast(
            Vector3 { origins[3 * i], origins[3 * i + 1], origins[3 * i + 2] },
            Vector3 { dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2] },
            radii[i], &normal, t_max[i]);
        t_out[i] = t;
        normals[3 * i] = normal.x;
        normals[3 * i + 1] = normal.y;
        normals[3 * i + 2] = normal.z;
    }
}

// per box: pMin, pMax; out: triangles visited, the fp32 sum of their vertices
// in visiting order, and FNV-1a over the visited vertices' words (the order)
SIM_API void mesh_cast_overlap(uint32_t family, uint32_t n, const float *boxes,
                               uint32_t *counts, float *sums, uint32_t *hashes)
{
    MeshBVH *bvh = probeTree(family);
    for (uint32_t i = 0; i < n; i++) {
        AABB box {
            Vector3 { boxes[6 * i], boxes[6 * i + 1], boxes[6 * i + 2] },
            Vector3 { boxes[6 * i + 3], boxes[6 * i + 4], boxes[6 * i + 5] },
        };
        uint32_t count = 0;
        uint32_t hash = 2166136261u;
        Vector3 sum { 0.f, 0.f, 0.f };
        bvh->findOverlaps(box, [&](Vector3 a, Vector3 b, Vector3 c) {
            count++;
            const Vector3 tri[3] = { a, b, c };
            for (const Vector3 &v : tri) {
                sum = sum + v;
                uint32_t words[3];
                memcpy(words, &v, sizeof(words));
                for (uint32_t w : words) {
                    hash = (hash ^ w) * 16777619u;
                }
            }
        });
        counts[i] = count;
        sums[3 * i] = sum.x;
        sums[3 * i + 1] = sum.y;
        sums[3 * i + 2] = sum.z;
        hashes[i] = hash;
    }
}

// QBVHNode::construct over n child sets (4 boxes of 6 floats and 4 indices
// each, num_children[i] of them used) and convertToAABB of every slot of the
// result (4 boxes of 6 floats per node)
SIM_API void mesh_cast_construct(uint32_t n, const uint32_t *num_children,
                                 const float *aabbs, const int32_t *indices,
                                 void *nodes_out, float *boxes_out)
{
    for (uint32_t i = 0; i < n; i++) {
        AABB boxes[4];
        int32_t idx[4];
        memcpy(boxes, aabbs + 24 * i, sizeof(boxes));
        memcpy(idx, indices + 4 * i, sizeof(idx));
        QBVHNode node = QBVHNode::construct(num_children[i], boxes, idx);
        memcpy((char *)nodes_out + sizeof(QBVHNode) * i, &node,
               sizeof(QBVHNode));
        for (uint32_t c = 0; c < 4; c++) {
            AABB box = node.convertToAABB(c);
            memcpy(boxes_out + 24 * i + 6 * c, &box, sizeof(box));
        }
    }
}

}
