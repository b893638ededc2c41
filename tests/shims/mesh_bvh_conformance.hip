// TEST INFRASTRUCTURE.  API conformance of <madrona/mesh_bvh.hpp>, device side:
// a translation unit wrapped like a simulator's (user prelude, then the
// force_cuda_host_device pragma) whose kernel names every member the header
// gained with the queries.  A missing or mis-declared one fails the build; the
// host half is mesh_bvh_conformance_host.cpp, the test
// tests/test_mesh_bvh_cpu.py.
#include <madrona/mwhip/user_prelude.hpp>
#pragma clang force_cuda_host_device begin
#include <madrona/mesh_bvh.hpp>

#ifndef MADRONA_COMPRESSED_DEINDEXED_TEX
#error "mesh_bvh.hpp must define MADRONA_COMPRESSED_DEINDEXED_TEX"
#endif

using namespace madrona;
using namespace madrona::math;

namespace meshbvhconf {

inline float touchMeshBVH(MeshBVH &bvh, Vector3 o, Vector3 d)
{
    int32_t stack[32];
    int32_t stack_size = 0;
    MeshBVH::HitInfo hit {};
    bool did_hit = bvh.traceRay(o, d, &hit, stack, stack_size);
    did_hit |= bvh.traceRay(o, d, &hit, stack, stack_size, 4.f);

    Diag3x3 inv_d = Diag3x3::fromVec(d).inv();
    MeshBVH::RayIsectTxfm txfm = bvh.computeRayIsectTxfm(o, d, inv_d);
    MeshBVH::RayIsectTxfm txfm2 =
        MeshBVH::computeRayIsectTxfm(o, d, inv_d, bvh.rootAABB);
    did_hit |= bvh.traceRayLeaf(0, 1, txfm, o, FLT_MAX, &hit);

    Vector3 a, b, c, bary, normal;
    Vector2 uva, uvb, uvc;
    bool fetched = bvh.fetchLeafTriangle(0, 0, &a, &b, &c, &uva, &uvb, &uvc);
    float tri_t = 0.f;
    did_hit |= bvh.rayTriangleIntersection(a, b, c, txfm2.kx, txfm2.ky,
        txfm2.kz, txfm2.Sx, txfm2.Sy, txfm2.Sz, o, FLT_MAX, &tri_t, &bary,
        &normal);

    Vector3 sweep_n { 0.f, 0.f, 0.f };
    float t = bvh.sphereCast(o, d, 0.25f, &sweep_n);
    t += bvh.sphereCast(o, d, 0.25f, &sweep_n, 1.f);
    bool near = bvh.sphereCastNodeCheck(o, inv_d, 1.f, 0.25f, bvh.rootAABB);
    t += bvh.sphereCastLeaf(0, o, d, 1.f, 0.25f, &sweep_n);
    t += bvh.sphereCastTriangle(a, b, c, o, d, 1.f, 0.25f, &sweep_n);

    uint32_t visited = 0;
    bvh.findOverlaps(bvh.rootAABB, [&](Vector3, Vector3, Vector3) {
        visited++;
    });

    uint32_t mat = bvh.getMaterialIDX(hit) + bvh.getMaterialIDX((int32_t)0);

    AABB boxes[2] = { bvh.rootAABB, bvh.nodes[0].convertToAABB(0) };
    int32_t idx[2] = { -1, 2 };
    QBVHNode node = QBVHNode::construct(2, boxes, idx);
    TriangleIndices tri_idx { { 0, 1, 2 } };
    Vector3 q = geo::triangleClosestPointToOrigin(a, b, c, b - a, c - a);

    return t + tri_t + q.x + txfm.oNear.x + txfm.oFar.y + txfm.invDirNear.z +
        txfm.invDirFar.x + hit.tHit + hit.normal.x + hit.uv.x +
        (float)(mat + visited + hit.leafMaterialIDX + tri_idx.indices[2] +
                (uint32_t)node.numChildren + (node.hasChild(1) ? 1u : 0u) +
                (node.isLeaf(0) ? 1u : 0u) + node.leafIDX(0) +
                (did_hit ? 1u : 0u) + (fetched ? 1u : 0u) + (near ? 1u : 0u) +
                (uint32_t)(txfm.nearX + txfm.nearY + txfm.nearZ + txfm.farX +
                           txfm.farY + txfm.farZ) +
                (uint32_t)(MeshBVH::sentinel == -1) +
                (uint32_t)(hit.bvh == nullptr) +
                (uint32_t)MeshBVH::numTrisPerLeaf + (uint32_t)MeshBVH::nodeWidth);
}

}
#pragma clang force_cuda_host_device end

__global__ void meshBVHConformanceKernel(MeshBVH *bvh, Vector3 *rays,
                                         float *out)
{
    out[threadIdx.x] = meshbvhconf::touchMeshBVH(*bvh, rays[2 * threadIdx.x],
                                                 rays[2 * threadIdx.x + 1]);
}
