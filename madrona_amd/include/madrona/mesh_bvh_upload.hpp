// A host MeshBVH (MeshBVHBuilder::build) copied to the device, for a Manager
// that hands meshes to its simulator's Config.  Host only; an extension (the
// reference's simulators run MeshBVHs through its renderer's asset path).
//
// One allocation holds the three arrays, each at an offset that is a multiple
// of 128 bytes (meshBVHUploadLayout): the nodes, the per-triangle materials,
// and the vertices with their padded tail of numTrisPerLeaf - 1 triangles
// (mesh_bvh_builder.hpp, guarantee 6).  The returned struct is the host one
// with its three pointers into that block; nodes is the block's base.  Runs
// over mwhip_raw_alloc / mwhip_raw_copy_h2d, so it works before an executor
// exists.
#pragma once

#include <madrona/mesh_bvh.hpp>
#include <mwhip.h>

#include <cstdlib>
#include <vector>
#include <cstring>

namespace madrona {

struct MeshBVHUploadLayout {
    uint64_t nodesOffset;       // 0
    uint64_t leafMatsOffset;
    uint64_t verticesOffset;
    uint64_t numVertexBytes;    // with the padded tail
    uint64_t numBytes;
};

inline MeshBVHUploadLayout meshBVHUploadLayout(const MeshBVH &host)
{
    auto align = [](uint64_t v) { return (v + 127u) & ~(uint64_t)127u; };
    uint64_t num_tris = host.numVerts / 3;
    MeshBVHUploadLayout l;
    l.nodesOffset = 0;
    l.leafMatsOffset = align(sizeof(QBVHNode) * (uint64_t)host.numNodes);
    l.verticesOffset = align(l.leafMatsOffset +
        sizeof(MeshBVH::LeafMaterial) * num_tris);
    l.numVertexBytes = sizeof(MeshBVH::BVHVertex) * 3 *
        (num_tris + (uint64_t)MeshBVH::numTrisPerLeaf - 1);
    l.numBytes = align(l.verticesOffset + l.numVertexBytes);
    return l;
}

// nodes == nullptr on failure
inline MeshBVH uploadMeshBVH(int gpu_id, const MeshBVH &host)
{
    MeshBVH dev = host;
    dev.nodes = nullptr;
    dev.leafMats = nullptr;
    dev.vertices = nullptr;
    if (host.nodes == nullptr) {
        return dev;
    }

    MeshBVHUploadLayout l = meshBVHUploadLayout(host);

    // staged so that the block's gaps are defined bytes too
    std::vector<char> staging(l.numBytes, 0);
    memcpy(staging.data() + l.nodesOffset, host.nodes,
           sizeof(QBVHNode) * (uint64_t)host.numNodes);
    memcpy(staging.data() + l.leafMatsOffset, host.leafMats,
           sizeof(MeshBVH::LeafMaterial) * (uint64_t)(host.numVerts / 3));
    memcpy(staging.data() + l.verticesOffset, host.vertices,
           l.numVertexBytes);

    char *block = (char *)mwhip_raw_alloc(gpu_id, l.numBytes);
    if (block == nullptr) {
        return dev;
    }
    if (mwhip_raw_copy_h2d(gpu_id, block, staging.data(), l.numBytes) != 0) {
        mwhip_raw_free(gpu_id, block);
        return dev;
    }

    dev.nodes = (QBVHNode *)(block + l.nodesOffset);
    dev.leafMats = (MeshBVH::LeafMaterial *)(block + l.leafMatsOffset);
    dev.vertices = (MeshBVH::BVHVertex *)(block + l.verticesOffset);
    return dev;
}

inline void freeUploadedMeshBVH(int gpu_id, MeshBVH &dev)
{
    if (dev.nodes != nullptr) {
        mwhip_raw_free(gpu_id, dev.nodes);
    }
    dev = MeshBVH {};
}

}
