// Bottom-level triangle-mesh BVH: the layouts a renderer hands to the batch ray
// caster (reference include/madrona/mesh_bvh.hpp:20-47, 146-178, 294-307: the
// 4-wide quantised node, the per-triangle material record, the de-indexed
// vertex with its uv, the Material record, the MeshBVH header) and the queries
// a simulator runs against static geometry (reference mesh_bvh.hpp:49-127,
// 158-292, mesh_bvh.inl): traceRay, sphereCast, findOverlaps, getMaterialIDX,
// QBVHNode::construct / convertToAABB.  The queries live in mesh_bvh.inl and
// run on the host and per lane on the device; the layouts are unchanged, the
// ray caster still reads them as raw memory (madrona/mw_gpu.hpp).
//
// Trees come from MeshBVHBuilder::build (madrona/mesh_bvh_builder.hpp, host)
// and reach the device through uploadMeshBVH (madrona/mesh_bvh_upload.hpp).
//
// Stack depth.  sphereCast and findOverlaps walk depth first with a 32-entry
// stack of their own; traceRay pushes onto the caller's stack, above the
// stack_size it is handed.  A pop is followed by at most nodeWidth pushes, so
// a tree whose internal nodes are at most D levels deep needs
// 3 * (D - 1) + 1 entries: D <= 11 for the 32 entries of the two fixed
// stacks, which MeshBVHBuilder guarantees, and traceRay's caller provides
// stack_size + 3 * (D - 1) + 1 entries (32 above stack_size always suffice
// for a tree of MeshBVHBuilder's).  Nothing checks the bound at run time.
#pragma once

#include <madrona/types.hpp>
#include <madrona/math.hpp>
#include <madrona/geo.hpp>

#include <cstddef>

#define MADRONA_COMPRESSED_DEINDEXED_TEX

#define MADRONA_BVH_WIDTH 4

#ifndef MADRONA_BLAS_LEAF_WIDTH
#define MADRONA_BLAS_LEAF_WIDTH 2
#endif

namespace madrona {

template <typename NodeIndex, int Width>
struct BVHNodeQuantized {
    using BVHNodeT = BVHNodeQuantized<NodeIndex, Width>;
    using NodeIndexT = NodeIndex;
    static constexpr int NodeWidth = Width;

    math::Vector3 minPoint;
    int8_t expX, expY, expZ;
    uint8_t numChildren;
    // bottom level: triangles of each leaf child
    uint8_t triSize[Width];
    // child boxes, quantised to 8 bits against minPoint / 2^exp
    uint8_t qMinX[Width], qMinY[Width], qMinZ[Width];
    uint8_t qMaxX[Width], qMaxY[Width], qMaxZ[Width];
    // internal child: its node index; leaf: 0x80000000 | first triangle;
    // 0xFFFFFFFF: no such child
    NodeIndex childrenIdx[Width];

    // child box i, dequantised: minPoint + 2^exp * q per axis
    MADRONA_HD inline math::AABB convertToAABB(uint32_t child_idx) const;

    // The node over num_children boxes.  child_indices: > 0 an internal
    // node's index + 1, < 0 -(first triangle of a leaf) - 1.  triSize is left
    // for the caller.  The exponent of an axis is clamped to [-126, 127], so
    // an axis of zero extent gets 2^-126 (a normal float) and q = 0 where the
    // reference's formula converts log2f(0) = -inf to int8_t.
    MADRONA_HD static inline BVHNodeT construct(uint32_t num_children,
                                                math::AABB *child_aabbs,
                                                int32_t *child_indices);

    MADRONA_HD bool hasChild(uint32_t i) const { return childrenIdx[i] != 0xFFFF'FFFFu; }
    MADRONA_HD bool isLeaf(uint32_t i) const { return (childrenIdx[i] & 0x8000'0000u) != 0u; }
    MADRONA_HD uint32_t leafIDX(uint32_t i) const { return childrenIdx[i] & ~0x8000'0000u; }
};

using QBVHNode = BVHNodeQuantized<uint32_t, MADRONA_BVH_WIDTH>;
static_assert(sizeof(QBVHNode) == 12 + 4 + 4 + 24 + 16);

struct Material {
    math::Vector4 color;
    int32_t textureIdx;     // -1: untextured
    float roughness;
    float metalness;
};

struct TriangleIndices {
    uint32_t indices[3];
};

struct MeshBVH {
    static constexpr inline CountT numTrisPerLeaf = MADRONA_BLAS_LEAF_WIDTH;
    static constexpr inline CountT nodeWidth = MADRONA_BVH_WIDTH;
    static constexpr inline int32_t sentinel = (int32_t)0xFFFF'FFFF;

    struct BVHMaterial {
        int32_t matIDX;
    };

    struct LeafMaterial {
        BVHMaterial material[1];
    };

    struct BVHVertex {
        math::Vector3 pos;
        math::Vector2 uv;
    };

    // per-ray constants of the watertight triangle test (Woop et al. 2013)
    struct RayIsectTxfm {
        int32_t kx;
        int32_t ky;
        int32_t kz;
        float Sx;
        float Sy;
        float Sz;
        int32_t nearX;
        int32_t nearY;
        int32_t nearZ;
        int32_t farX;
        int32_t farY;
        int32_t farZ;
        math::Vector3 oNear;
        math::Vector3 oFar;
        math::Vector3 invDirNear;
        math::Vector3 invDirFar;
    };

    struct HitInfo {
        float tHit;
        math::Vector3 normal;
        math::Vector2 uv;

        MeshBVH *bvh;       // not written by traceRay

        uint32_t leafMaterialIDX;
    };

    // fn(a, b, c) for every triangle of every leaf whose box overlaps aabb,
    // in traversal order
    template <typename Fn>
    MADRONA_HD void findOverlaps(const math::AABB &aabb, Fn &&fn) const;

    // Closest front-facing hit below t_max (back faces are culled).  stack:
    // see "Stack depth" above; stack_size is the same on return.
    MADRONA_HD inline bool traceRay(math::Vector3 ray_o,
                                    math::Vector3 ray_d,
                                    HitInfo *out_hit_info,
                                    int32_t *stack,
                                    int32_t &stack_size,
                                    float t_max = float(FLT_MAX)) const;

    // Sweeps a sphere of radius sphere_r from ray_o along ray_d (not
    // normalised: t = 1 is the whole move).  Returns the first contact's t,
    // or t_max; the normal is written only when t < t_max.
    MADRONA_HD inline float sphereCast(math::Vector3 ray_o,
                                       math::Vector3 ray_d,
                                       float sphere_r,
                                       math::Vector3 *out_hit_normal,
                                       float t_max = float(FLT_MAX));

    MADRONA_HD inline bool traceRayLeaf(
        int32_t leaf_idx,
        int32_t num_tris,
        RayIsectTxfm tri_isect_txfm,
        math::Vector3 ray_o,
        float t_max,
        HitInfo *hit_info) const;

    MADRONA_HD inline bool rayTriangleIntersection(
        math::Vector3 tri_a, math::Vector3 tri_b, math::Vector3 tri_c,
        int32_t kx, int32_t ky, int32_t kz,
        float Sx, float Sy, float Sz,
        math::Vector3 org,
        float t_max,
        float *out_hit_t,
        math::Vector3 *bary_out,
        math::Vector3 *out_hit_normal) const;

    // triangle leaf_idx + offset; always succeeds (see sphereCastLeaf)
    MADRONA_HD inline bool fetchLeafTriangle(CountT leaf_idx,
                                             CountT offset,
                                             math::Vector3 *a,
                                             math::Vector3 *b,
                                             math::Vector3 *c,
                                             math::Vector2 *uv_a,
                                             math::Vector2 *uv_b,
                                             math::Vector2 *uv_c) const;

    MADRONA_HD static inline RayIsectTxfm computeRayIsectTxfm(
        math::Vector3 o, math::Vector3 d, math::Diag3x3 inv_d,
        math::AABB root_aabb);

    MADRONA_HD inline RayIsectTxfm computeRayIsectTxfm(
        math::Vector3 o, math::Vector3 d, math::Diag3x3 inv_d) const;

    MADRONA_HD inline bool sphereCastNodeCheck(math::Vector3 ray_o,
                                               math::Diag3x3 inv_d,
                                               float t_max,
                                               float sphere_r,
                                               math::AABB aabb) const;

    MADRONA_HD inline float sphereCastLeaf(int32_t leaf_idx,
                                           math::Vector3 ray_o,
                                           math::Vector3 ray_d,
                                           float t_max,
                                           float sphere_r,
                                           math::Vector3 *out_hit_normal) const;

    MADRONA_HD inline float sphereCastTriangle(math::Vector3 tri_a,
                                               math::Vector3 tri_b,
                                               math::Vector3 tri_c,
                                               math::Vector3 ray_o,
                                               math::Vector3 ray_d,
                                               float t_max,
                                               float sphere_r,
                                               math::Vector3 *out_hit_normal) const;

    MADRONA_HD inline uint32_t getMaterialIDX(const HitInfo &info) const;
    MADRONA_HD inline uint32_t getMaterialIDX(int32_t mat_idx) const;

    QBVHNode *nodes;
    LeafMaterial *leafMats;     // per triangle, read when materialIDX == -1
    BVHVertex *vertices;        // 3 per triangle, leaf order

    math::AABB rootAABB;
    uint32_t numNodes;
    uint32_t numLeaves;
    uint32_t numVerts;

    int32_t materialIDX;        // the whole mesh's material, or -1: per triangle

    uint32_t magic;
};

// the batch ray caster reads these structs as raw memory
static_assert(sizeof(MeshBVH) == 72);
static_assert(offsetof(MeshBVH, nodes) == 0);
static_assert(offsetof(MeshBVH, leafMats) == 8);
static_assert(offsetof(MeshBVH, vertices) == 16);
static_assert(offsetof(MeshBVH, rootAABB) == 24);
static_assert(offsetof(MeshBVH, numNodes) == 48);
static_assert(offsetof(MeshBVH, numLeaves) == 52);
static_assert(offsetof(MeshBVH, numVerts) == 56);
static_assert(offsetof(MeshBVH, materialIDX) == 60);
static_assert(offsetof(MeshBVH, magic) == 64);
static_assert(sizeof(MeshBVH::BVHVertex) == 20);
static_assert(sizeof(MeshBVH::LeafMaterial) == 4);

}

#include "mesh_bvh.inl"
