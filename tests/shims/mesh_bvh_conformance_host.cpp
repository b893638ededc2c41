// TEST INFRASTRUCTURE.  Host half of the MeshBVH API conformance check (see
// mesh_bvh_conformance.hip): the builder, the uploader's layout and the
// queries named from plain host C++, and the struct layout of the reference's
// mesh_bvh.hpp reported for the test.
#include <madrona/mesh_bvh.hpp>
#include <madrona/mesh_bvh_builder.hpp>
#include <madrona/mesh_bvh_upload.hpp>

#include <cstddef>

using namespace madrona;

extern "C" {

#define API __attribute__((visibility("default")))

// out[24]: see tests/test_mesh_bvh_cpu.py::test_conformance
API void meshbvhconf_layout(uint64_t *out)
{
    out[0] = sizeof(QBVHNode);
    out[1] = sizeof(MeshBVH);
    out[2] = offsetof(MeshBVH, nodes);
    out[3] = offsetof(MeshBVH, leafMats);
    out[4] = offsetof(MeshBVH, vertices);
    out[5] = offsetof(MeshBVH, rootAABB);
    out[6] = offsetof(MeshBVH, numNodes);
    out[7] = offsetof(MeshBVH, numLeaves);
    out[8] = offsetof(MeshBVH, numVerts);
    out[9] = offsetof(MeshBVH, materialIDX);
    out[10] = offsetof(MeshBVH, magic);
    out[11] = sizeof(MeshBVH::BVHVertex);
    out[12] = sizeof(MeshBVH::LeafMaterial);
    out[13] = sizeof(MeshBVH::RayIsectTxfm);
    out[14] = sizeof(MeshBVH::HitInfo);
    out[15] = offsetof(MeshBVH::HitInfo, tHit);
    out[16] = offsetof(MeshBVH::HitInfo, normal);
    out[17] = offsetof(MeshBVH::HitInfo, uv);
    out[18] = offsetof(MeshBVH::HitInfo, bvh);
    out[19] = offsetof(MeshBVH::HitInfo, leafMaterialIDX);
    out[20] = sizeof(TriangleIndices);
    out[21] = (uint64_t)MeshBVH::numTrisPerLeaf;
    out[22] = (uint64_t)MeshBVH::nodeWidth;
    out[23] = (uint32_t)MeshBVH::sentinel;
}

// One triangle through the host API: built, laid out for upload, hit by a ray
// from above and missed from below (back face), swept onto, overlapped.
// Returns 1 when all of that holds.
API uint32_t meshbvhconf_host_queries()
{
    math::Vector3 positions[3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 0, 1, 0 } };
    uint32_t indices[3] = { 0, 1, 2 };
    imp::SourceMesh src {};
    src.positions = positions;
    src.indices = indices;
    src.numVertices = 3;
    src.numFaces = 1;
    src.materialIDX = 7;

    MeshBVH bvh = MeshBVHBuilder::build(Span<const imp::SourceMesh>(&src, 1));
    bool ok = bvh.numNodes == 1 && bvh.numLeaves == 1 && bvh.numVerts == 3;

    MeshBVHUploadLayout layout = meshBVHUploadLayout(bvh);
    ok = ok && layout.leafMatsOffset % 128 == 0 &&
        layout.verticesOffset % 128 == 0 && layout.numBytes % 128 == 0;

    int32_t stack[32];
    int32_t stack_size = 0;
    MeshBVH::HitInfo hit {};
    ok = ok && bvh.traceRay({ 0.25f, 0.25f, 2.f }, { 0, 0, -1 }, &hit, stack,
                            stack_size);
    ok = ok && hit.tHit == 2.f && bvh.getMaterialIDX(hit) == 7 &&
        stack_size == 0;
    ok = ok && !bvh.traceRay({ 0.25f, 0.25f, -2.f }, { 0, 0, 1 }, &hit, stack,
                             stack_size);

    math::Vector3 normal { 0, 0, 0 };
    float t = bvh.sphereCast({ 0.25f, 0.25f, 2.f }, { 0, 0, -4 }, 0.5f,
                             &normal, 1.f);
    ok = ok && t == 0.375f && normal.z == 1.f;

    uint32_t visited = 0;
    bvh.findOverlaps(math::AABB { { -1, -1, -1 }, { 2, 2, 1 } },
        [&](math::Vector3, math::Vector3, math::Vector3) { visited++; });
    ok = ok && visited == 1;

    MeshBVHBuilder::free(bvh);
    return ok && bvh.nodes == nullptr ? 1u : 0u;
}

// Builds num_tris triangles (9 floats each) and returns the tree's node count
// (0: build returned an empty MeshBVH).
API uint32_t meshbvhconf_build_nodes(const float *positions, uint32_t num_tris)
{
    std::vector<uint32_t> indices(3 * (size_t)num_tris);
    for (size_t i = 0; i < indices.size(); i++) {
        indices[i] = (uint32_t)i;
    }
    imp::SourceMesh src {};
    src.positions = (math::Vector3 *)positions;
    src.indices = indices.data();
    src.numVertices = 3 * num_tris;
    src.numFaces = num_tris;

    MeshBVH bvh = MeshBVHBuilder::build(Span<const imp::SourceMesh>(&src, 1));
    uint32_t num_nodes = bvh.nodes == nullptr ? 0u : bvh.numNodes;
    MeshBVHBuilder::free(bvh);
    return num_nodes;
}

}
