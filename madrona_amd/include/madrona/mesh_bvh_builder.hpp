// MeshBVHBuilder::build: the bottom-level tree MeshBVH's queries walk, from
// source meshes.  Host only.  API contract: reference
// include/madrona/mesh_bvh_builder.hpp:7-11.
//
// The reference builds with Embree (src/common/mesh_bvh_builder.cpp); the
// tree's SHAPE here is this backend's own, a 4-wide median split:
//   a node over n triangles covers ceil(n / numTrisPerLeaf) leaves.  Up to
//   four leaves: they are its children.  More: the triangles are sorted by
//   centroid along the longest axis of their centroids' bounds and cut in two
//   at a leaf boundary, each half once more along its own longest axis, and
//   the four quarters are the children (a quarter of one leaf is a leaf).
// What is emitted is what the reference emits (mesh_bvh_builder.cpp:545-554,
// 673-738): at most numTrisPerLeaf triangles per leaf, a leaf child's index
// 0x80000000 | its first triangle and its triSize, vertices de-indexed in leaf
// order with their uvs, one LeafMaterial per triangle (the face's material,
// or the mesh's where it has no per-face ones), materialIDX = -1.
//
// Guarantees (tests/test_mesh_bvh_cpu.py):
//   1. every child box, dequantised (QBVHNode::convertToAABB), contains every
//      vertex beneath it: the quantised bounds are checked against the exact
//      ones and moved outwards where fp32 rounding left them inside;
//   2. rootAABB is the exact bounds of the mesh;
//   3. numNodes / numLeaves / numVerts are consistent, 1 <= triSize <=
//      numTrisPerLeaf, unused children are 0xFFFFFFFF with zero bytes;
//   4. internal nodes are at most 11 levels deep (the 32-entry stacks of
//      sphereCast / findOverlaps, see mesh_bvh.hpp).  Every level divides the
//      number of leaves by four, rounding up, so this holds for up to 4^11
//      leaves; build returns an empty MeshBVH (nodes == nullptr) beyond;
//      (input domain: build also returns an empty MeshBVH for a mesh with no
//      triangle, with a non-finite position, or whose bounds' extent
//      overflows fp32 -- the quantisation has no exponent for those)
//   5. exponents are clamped to >= -126: an axis of zero extent (a floor quad)
//      gets the smallest normal scale 2^-126 and q = 0, all finite;
//   6. the vertex array is followed by numTrisPerLeaf - 1 copies of the last
//      triangle, not counted in numVerts (MeshBVH::sphereCastLeaf reads them);
//   7. a single triangle gives one node with one leaf child.
//
// The exponent is found by comparing against 255 * 2^e, not through log2f, so
// the same bytes come out wherever this is compiled.  This header uses only
// names the reference's headers define too, so a simulator's reference-CPU
// build gets the identical tree by including this file by path.
//
// Extension: MeshBVHBuilder::free releases what build returned (the reference
// leaves the arrays to the caller without saying how they were allocated).
#pragma once

#include <madrona/mesh_bvh.hpp>
#include <madrona/importer.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace madrona {

struct MeshBVHBuilder {
    static inline MeshBVH build(Span<const imp::SourceMesh> src_meshes);

    // extension, see above
    static inline void free(MeshBVH &bvh);

    static constexpr inline uint32_t maxDepth = 11;

private:
    struct Tri {
        math::Vector3 pos[3];
        math::Vector2 uv[3];
        int32_t material;
        math::Vector3 centroid;
        uint32_t order;     // input order: the sort's tie break
    };

    struct Ctx {
        std::vector<Tri> tris;
        std::vector<QBVHNode> nodes;
        uint32_t numLeaves;
    };

    static inline math::AABB boundsOf(const Ctx &ctx, uint32_t begin,
                                      uint32_t end)
    {
        math::AABB box {
            { INFINITY, INFINITY, INFINITY },
            { -INFINITY, -INFINITY, -INFINITY },
        };
        for (uint32_t i = begin; i < end; i++) {
            for (const math::Vector3 &p : ctx.tris[i].pos) {
                box.pMin.x = fminf(box.pMin.x, p.x);
                box.pMin.y = fminf(box.pMin.y, p.y);
                box.pMin.z = fminf(box.pMin.z, p.z);
                box.pMax.x = fmaxf(box.pMax.x, p.x);
                box.pMax.y = fmaxf(box.pMax.y, p.y);
                box.pMax.z = fmaxf(box.pMax.z, p.z);
            }
        }
        return box;
    }

    // sorts [begin, end) along the longest axis of the centroids' bounds
    static inline void sortRange(Ctx &ctx, uint32_t begin, uint32_t end)
    {
        float lo[3] = { INFINITY, INFINITY, INFINITY };
        float hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (uint32_t i = begin; i < end; i++) {
            const math::Vector3 &c = ctx.tris[i].centroid;
            float v[3] = { c.x, c.y, c.z };
            for (int a = 0; a < 3; a++) {
                lo[a] = fminf(lo[a], v[a]);
                hi[a] = fmaxf(hi[a], v[a]);
            }
        }
        int axis = 0;
        for (int a = 1; a < 3; a++) {
            if (hi[a] - lo[a] > hi[axis] - lo[axis]) {
                axis = a;
            }
        }
        std::sort(ctx.tris.begin() + begin, ctx.tris.begin() + end,
            [axis](const Tri &a, const Tri &b) {
                float ka = axis == 0 ? a.centroid.x :
                    (axis == 1 ? a.centroid.y : a.centroid.z);
                float kb = axis == 0 ? b.centroid.x :
                    (axis == 1 ? b.centroid.y : b.centroid.z);
                if (ka != kb) {
                    return ka < kb;
                }
                return a.order < b.order;
            });
    }

    // one axis of a node: the exponent (smallest e >= -126 with 255 * 2^e >=
    // extent) and the children's quantised bounds, checked against the exact
    // ones; returns false if a bound does not fit in 8 bits at this exponent
    static inline bool quantiseAxis(int32_t e, float node_min,
                                    const float *child_lo,
                                    const float *child_hi,
                                    uint32_t num_children,
                                    uint8_t *q_lo, uint8_t *q_hi)
    {
        float scale = ldexpf(1.f, e);
        for (uint32_t i = 0; i < num_children; i++) {
            float fl = floorf((child_lo[i] - node_min) / scale);
            float fh = ceilf((child_hi[i] - node_min) / scale);
            if (!(fl >= 0.f)) fl = 0.f;
            if (!(fh >= 0.f)) fh = 0.f;
            if (fl > 255.f) fl = 255.f;
            while (fl > 0.f && node_min + scale * fl > child_lo[i]) {
                fl -= 1.f;
            }
            while (fh <= 255.f && node_min + scale * fh < child_hi[i]) {
                fh += 1.f;
            }
            if (fh > 255.f) {
                return false;
            }
            q_lo[i] = (uint8_t)fl;
            q_hi[i] = (uint8_t)fh;
        }
        return true;
    }

    static inline int8_t quantiseAxisAnyExp(float node_min, float node_max,
                                            const float *child_lo,
                                            const float *child_hi,
                                            uint32_t num_children,
                                            uint8_t *q_lo, uint8_t *q_hi)
    {
        float extent = node_max - node_min;
        int32_t e = -126;
        while (e < 127 && ldexpf(255.f, e) < extent) {
            e++;
        }
        while (e < 127 && !quantiseAxis(e, node_min, child_lo, child_hi,
                                        num_children, q_lo, q_hi)) {
            e++;
        }
        return (int8_t)e;
    }

    // the node over [begin, end), more than one leaf's worth of triangles or
    // the root; returns its index
    static inline uint32_t buildNode(Ctx &ctx, uint32_t begin, uint32_t end)
    {
        constexpr uint32_t L = (uint32_t)MeshBVH::numTrisPerLeaf;
        constexpr uint32_t W = (uint32_t)MeshBVH::nodeWidth;

        uint32_t node_idx = (uint32_t)ctx.nodes.size();
        ctx.nodes.push_back(QBVHNode {});

        uint32_t n = end - begin;
        uint32_t num_leaves = (n + L - 1) / L;

        // child ranges
        uint32_t cuts[W + 1];
        uint32_t num_children;
        sortRange(ctx, begin, end);
        if (num_leaves <= W) {
            num_children = num_leaves;
            for (uint32_t i = 0; i < num_children; i++) {
                cuts[i] = begin + i * L;
            }
            cuts[num_children] = end;
        } else {
            num_children = W;
            uint32_t left_leaves = (num_leaves + 1) / 2;
            uint32_t mid = begin + left_leaves * L;
            sortRange(ctx, begin, mid);
            sortRange(ctx, mid, end);
            uint32_t ll = (left_leaves + 1) / 2;
            uint32_t rl = (num_leaves - left_leaves + 1) / 2;
            cuts[0] = begin;
            cuts[1] = begin + ll * L;
            cuts[2] = mid;
            cuts[3] = mid + rl * L;
            cuts[4] = end;
        }

        math::AABB boxes[W];
        uint32_t children[W];
        uint8_t tri_sizes[W];
        for (uint32_t i = 0; i < num_children; i++) {
            uint32_t b = cuts[i], e = cuts[i + 1];
            if (e - b <= L) {
                children[i] = 0x8000'0000u | b;
                tri_sizes[i] = (uint8_t)(e - b);
                ctx.numLeaves++;
            } else {
                children[i] = buildNode(ctx, b, e);
                tri_sizes[i] = 0;
            }
            // (after the recursion: it permutes [b, e) only within itself)
            boxes[i] = boundsOf(ctx, b, e);
        }

        QBVHNode node {};
        math::AABB all = boxes[0];
        for (uint32_t i = 1; i < num_children; i++) {
            all = math::AABB {
                { fminf(all.pMin.x, boxes[i].pMin.x),
                  fminf(all.pMin.y, boxes[i].pMin.y),
                  fminf(all.pMin.z, boxes[i].pMin.z) },
                { fmaxf(all.pMax.x, boxes[i].pMax.x),
                  fmaxf(all.pMax.y, boxes[i].pMax.y),
                  fmaxf(all.pMax.z, boxes[i].pMax.z) },
            };
        }
        node.minPoint = all.pMin;
        node.numChildren = (uint8_t)num_children;

        float lo[W], hi[W];
        for (uint32_t i = 0; i < num_children; i++) { lo[i] = boxes[i].pMin.x; hi[i] = boxes[i].pMax.x; }
        node.expX = quantiseAxisAnyExp(all.pMin.x, all.pMax.x, lo, hi,
                                       num_children, node.qMinX, node.qMaxX);
        for (uint32_t i = 0; i < num_children; i++) { lo[i] = boxes[i].pMin.y; hi[i] = boxes[i].pMax.y; }
        node.expY = quantiseAxisAnyExp(all.pMin.y, all.pMax.y, lo, hi,
                                       num_children, node.qMinY, node.qMaxY);
        for (uint32_t i = 0; i < num_children; i++) { lo[i] = boxes[i].pMin.z; hi[i] = boxes[i].pMax.z; }
        node.expZ = quantiseAxisAnyExp(all.pMin.z, all.pMax.z, lo, hi,
                                       num_children, node.qMinZ, node.qMaxZ);

        for (uint32_t i = 0; i < W; i++) {
            node.childrenIdx[i] = i < num_children ? children[i] : 0xFFFF'FFFFu;
            node.triSize[i] = i < num_children ? tri_sizes[i] : (uint8_t)0;
        }

        ctx.nodes[node_idx] = node;
        return node_idx;
    }
};

MeshBVH MeshBVHBuilder::build(Span<const imp::SourceMesh> src_meshes)
{
    constexpr uint32_t L = (uint32_t)MeshBVH::numTrisPerLeaf;

    Ctx ctx;
    ctx.numLeaves = 0;
    bool all_finite = true;

    for (const imp::SourceMesh &mesh : src_meshes) {
        uint32_t idx_offset = 0;
        for (uint32_t f = 0; f < mesh.numFaces; f++) {
            // polygons are fanned from their first vertex
            uint32_t face_verts =
                mesh.faceCounts != nullptr ? mesh.faceCounts[f] : 3u;
            const uint32_t *face = mesh.indices + idx_offset;
            idx_offset += face_verts;

            for (uint32_t k = 1; k + 1 < face_verts; k++) {
                uint32_t vi[3] = { face[0], face[k], face[k + 1] };
                Tri tri;
                for (int c = 0; c < 3; c++) {
                    tri.pos[c] = mesh.positions[vi[c]];
                    all_finite = all_finite && std::isfinite(tri.pos[c].x) &&
                        std::isfinite(tri.pos[c].y) &&
                        std::isfinite(tri.pos[c].z);
                    tri.uv[c] = mesh.uvs != nullptr ? mesh.uvs[vi[c]] :
                        math::Vector2 { 0.f, 0.f };
                }
                tri.material = (int32_t)(mesh.faceMaterials != nullptr ?
                    mesh.faceMaterials[f] : mesh.materialIDX);
                tri.centroid = (tri.pos[0] + tri.pos[1] + tri.pos[2]) *
                    (1.f / 3.f);
                tri.order = (uint32_t)ctx.tris.size();
                ctx.tris.push_back(tri);
            }
        }
    }

    MeshBVH bvh {};
    uint64_t num_tris = ctx.tris.size();
    // 4^maxDepth leaves
    if (num_tris == 0 || num_tris > (uint64_t)L * (1ull << (2 * maxDepth))) {
        return bvh;
    }

    // finite positions and a finite extent: every node's extent is then at
    // most 2^128, for which quantiseAxisAnyExp finds an exponent below 127
    math::AABB bounds = boundsOf(ctx, 0, (uint32_t)num_tris);
    math::Vector3 extent = bounds.pMax - bounds.pMin;
    if (!all_finite || !std::isfinite(extent.x) || !std::isfinite(extent.y) ||
            !std::isfinite(extent.z)) {
        return bvh;
    }

    buildNode(ctx, 0, (uint32_t)num_tris);

    uint64_t num_padded_tris = num_tris + (L - 1);
    auto *nodes = (QBVHNode *)malloc(sizeof(QBVHNode) * ctx.nodes.size());
    auto *mats = (MeshBVH::LeafMaterial *)malloc(
        sizeof(MeshBVH::LeafMaterial) * num_tris);
    auto *verts = (MeshBVH::BVHVertex *)malloc(
        sizeof(MeshBVH::BVHVertex) * 3 * num_padded_tris);

    memcpy(nodes, ctx.nodes.data(), sizeof(QBVHNode) * ctx.nodes.size());
    for (uint64_t t = 0; t < num_padded_tris; t++) {
        const Tri &tri = ctx.tris[t < num_tris ? t : num_tris - 1];
        for (int c = 0; c < 3; c++) {
            verts[3 * t + c].pos = tri.pos[c];
            verts[3 * t + c].uv = tri.uv[c];
        }
        if (t < num_tris) {
            mats[t].material[0].matIDX = tri.material;
        }
    }

    bvh.nodes = nodes;
    bvh.leafMats = mats;
    bvh.vertices = verts;
    bvh.rootAABB = bounds;
    bvh.numNodes = (uint32_t)ctx.nodes.size();
    bvh.numLeaves = ctx.numLeaves;
    bvh.numVerts = (uint32_t)(3 * num_tris);
    bvh.materialIDX = -1;
    bvh.magic = 0;
    return bvh;
}

void MeshBVHBuilder::free(MeshBVH &bvh)
{
    ::free(bvh.nodes);
    ::free(bvh.leafMats);
    ::free(bvh.vertices);
    bvh = MeshBVH {};
}

}
