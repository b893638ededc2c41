// TEST INFRASTRUCTURE.  <madrona/navmesh.hpp> on the device behind a C ABI
// for tests/test_navmesh_device_gpu.py:
//   * initFromPolygons, one lane per mesh, allocating from a persistent and a
//     scratch region of a stand-alone ecs_state (what a world constructor
//     sees), or the same meshes built on the host and copied over;
//   * one lane per query: samplePointAndPoly, then bfsFromPoly (centroid
//     within a radius of the sampled point, like navmesh_host_shim.cpp) and
//     dijkstrasFromPoly from the sampled polygon and point.  The search state
//     is global memory, max_tris entries per query.
#include <madrona/mwhip/user_prelude.hpp>
#include <madrona/navmesh.hpp>

#include <vector>

using namespace madrona;
using namespace madrona::math;

namespace {

struct PolyMesh {
    uint32_t vertOffset;    // into verts (Vector3)
    uint32_t idxOffset;     // into idxs (the mesh's poly offsets are relative)
    uint32_t polyOffset;    // into poly_offsets / poly_sizes
    uint32_t numVerts;
    uint32_t numPolys;
};

__global__ void __launch_bounds__(64)
buildKernel(const PolyMesh *meshes, uint32_t num_meshes, Vector3 *verts,
            uint32_t *idxs, uint32_t *poly_offsets, uint32_t *poly_sizes,
            Navmesh *out)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= num_meshes) {
        return;
    }
    PolyMesh pm = meshes[m];
    out[m] = Navmesh::initFromPolygons(verts + pm.vertOffset,
        idxs + pm.idxOffset, poly_offsets + pm.polyOffset,
        poly_sizes + pm.polyOffset, pm.numVerts, pm.numPolys);
}

struct QueryOut {
    float point[3];
    uint32_t poly;
    uint32_t bfsCount;
    uint32_t dijkstraCount;
};

__global__ void __launch_bounds__(64)
queryKernel(const Navmesh *meshes, const uint32_t *query_mesh,
            const RandKey *keys, uint32_t num_queries, uint32_t max_tris,
            float radius2, QueryOut *out, uint32_t *bfs_order,
            uint32_t *bfs_queue, bool *bfs_visited, float *distances,
            Vector3 *entries, uint32_t *heap, uint32_t *heap_index,
            uint32_t *pop_order, float *pop_dist)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= num_queries) {
        return;
    }
    Navmesh nav = meshes[query_mesh[q]];
    const uint64_t base = (uint64_t)q * max_tris;

    uint32_t poly;
    Vector3 pos = nav.samplePointAndPoly(keys[q], &poly);

    uint32_t bfs_count = 0;
    nav.bfsFromPoly(poly,
        Navmesh::BFSState { bfs_queue + base, bfs_visited + base },
        [&](uint32_t p) {
            bfs_order[base + bfs_count++] = p;
            Vector3 a, b, c;
            nav.getTriangleVertices(p, &a, &b, &c);
            Vector3 centroid = (a + b + c) * (1.f / 3.f);
            return (centroid - pos).length2() <= radius2;
        });

    Vector3 *entry = entries + base;
    for (uint32_t i = 0; i < nav.numTris; i++) {
        entry[i] = Vector3 { 0.f, 0.f, 0.f };
    }
    uint32_t pop_count = 0;
    nav.dijkstrasFromPoly(poly, pos,
        Navmesh::DijkstrasState { distances + base, entry, heap + base,
                                  heap_index + base },
        [&](uint32_t p, Vector3, float d) {
            pop_order[base + pop_count] = p;
            pop_dist[base + pop_count] = d;
            pop_count++;
        });

    QueryOut o;
    o.point[0] = pos.x;
    o.point[1] = pos.y;
    o.point[2] = pos.z;
    o.poly = poly;
    o.bfsCount = bfs_count;
    o.dijkstraCount = pop_count;
    out[q] = o;
}

template <typename T>
T *devCopy(const T *src, size_t n, std::vector<void *> &allocs)
{
    T *d = nullptr;
    if (hipMalloc(&d, sizeof(T) * (n > 0 ? n : 1)) != hipSuccess) {
        return nullptr;
    }
    allocs.push_back(d);
    if (n > 0) {
        (void)hipMemcpy(d, src, sizeof(T) * n, hipMemcpyHostToDevice);
    }
    return d;
}

template <typename T>
T *devAlloc(size_t n, std::vector<void *> &allocs)
{
    T *d = nullptr;
    if (hipMalloc(&d, sizeof(T) * (n > 0 ? n : 1)) != hipSuccess) {
        return nullptr;
    }
    allocs.push_back(d);
    (void)hipMemset(d, 0, sizeof(T) * (n > 0 ? n : 1));
    return d;
}

}

extern "C" {

#define API __attribute__((visibility("default")))

// meshes: num_meshes x { vert offset, idx offset, poly offset, verts, polys };
// tri_offsets[num_meshes + 1]: where each mesh's triangles start in the
// triangle outputs (the caller counts them: sum of poly sizes - 2).
// on_device: 1 builds with initFromPolygons on the device, 0 on the host (and
// copies the arrays over).
// Outputs per triangle: tri_idx[3], adjacency[3], tau, alias; per vertex:
// out_verts[3]; per query: query_out[6] (point xyz, poly, BFS count, Dijkstra
// count as raw words); per query x max_tris: bfs_order, pop_order, pop_dist,
// distances, entries[3].  persist_used[2]: bytes the device build took from
// the persistent and from the scratch region.
API int32_t nav_dev_run(const uint32_t *meshes, uint32_t num_meshes,
                        const float *verts, uint32_t num_verts,
                        const uint32_t *idxs, uint32_t num_idxs,
                        const uint32_t *poly_offsets, const uint32_t *poly_sizes,
                        uint32_t num_polys, const uint32_t *tri_offsets,
                        int32_t on_device,
                        const uint32_t *query_mesh, const uint32_t *keys,
                        uint32_t num_queries, uint32_t max_tris, float radius2,
                        uint32_t *tri_idx, uint32_t *adjacency, float *tau,
                        uint32_t *alias, float *out_verts, uint32_t *query_out,
                        uint32_t *bfs_order, uint32_t *pop_order,
                        float *pop_dist, float *distances, float *entries,
                        uint64_t *persist_used)
{
    std::vector<void *> allocs;
    auto cleanup = [&](int32_t rc) {
        for (void *p : allocs) {
            (void)hipFree(p);
        }
        return rc;
    };

    const PolyMesh *pms = (const PolyMesh *)meshes;
    const uint32_t total_tris = tri_offsets[num_meshes];
    std::vector<Navmesh> navs(num_meshes);
    persist_used[0] = 0;
    persist_used[1] = 0;

    if (on_device) {
        // a stand-alone ecs_state: just the two bump regions initFromPolygons
        // allocates from (no mailbox: neither region grows)
        uint64_t persist_bytes = 0, tmp_bytes = 0;
        for (uint32_t m = 0; m < num_meshes; m++) {
            uint32_t T = tri_offsets[m + 1] - tri_offsets[m];
            persist_bytes += navmesh_detail::deviceBlockBytes(pms[m].numVerts, T);
            tmp_bytes += (navmesh_detail::deviceTmpBytes(T) + 255) & ~255ull;
        }
        mwhip::EcsState hs {};
        hs.persistCapacity = persist_bytes + 4096;
        hs.tmpCapacity = tmp_bytes + 4096;
        hs.persistBase = devAlloc<char>(hs.persistCapacity, allocs);
        hs.tmpBase = devAlloc<char>(hs.tmpCapacity, allocs);
        mwhip::EcsState *d_state = devCopy(&hs, 1, allocs);
        if (hs.persistBase == nullptr || hs.tmpBase == nullptr ||
                d_state == nullptr) {
            return cleanup(-2);
        }
        void *state_ptr = d_state;
        if (hipMemcpyToSymbol(HIP_SYMBOL(mwGPU::deviceStateManager), &state_ptr,
                              sizeof(void *)) != hipSuccess) {
            return cleanup(-2);
        }

        PolyMesh *d_meshes = devCopy(pms, num_meshes, allocs);
        Vector3 *d_verts = devCopy((const Vector3 *)verts, num_verts, allocs);
        uint32_t *d_idxs = devCopy(idxs, num_idxs, allocs);
        uint32_t *d_offs = devCopy(poly_offsets, num_polys, allocs);
        uint32_t *d_sizes = devCopy(poly_sizes, num_polys, allocs);
        Navmesh *d_navs = devAlloc<Navmesh>(num_meshes, allocs);
        hipLaunchKernelGGL(buildKernel, dim3((num_meshes + 63) / 64), dim3(64),
                           0, 0, d_meshes, num_meshes, d_verts, d_idxs, d_offs,
                           d_sizes, d_navs);
        if (hipDeviceSynchronize() != hipSuccess) {
            return cleanup(-3);
        }
        (void)hipMemcpy(navs.data(), d_navs, sizeof(Navmesh) * num_meshes,
                        hipMemcpyDeviceToHost);
        mwhip::EcsState after {};
        (void)hipMemcpy(&after, d_state, sizeof(after), hipMemcpyDeviceToHost);
        if (after.errorFlags != 0) {
            return cleanup(-4);
        }
        persist_used[0] = after.persistOffset;
        persist_used[1] = after.tmpOffset;
    } else {
        for (uint32_t m = 0; m < num_meshes; m++) {
            const PolyMesh &pm = pms[m];
            Navmesh host = Navmesh::initFromPolygons(
                (Vector3 *)verts + pm.vertOffset,
                (uint32_t *)idxs + pm.idxOffset,
                (uint32_t *)poly_offsets + pm.polyOffset,
                (uint32_t *)poly_sizes + pm.polyOffset,
                pm.numVerts, pm.numPolys);
            Navmesh &dev = navs[m];
            dev = host;
            dev.vertices = devCopy(host.vertices, host.numVerts, allocs);
            dev.triIndices = devCopy(host.triIndices, 3 * host.numTris, allocs);
            dev.triAdjacency = devCopy(host.triAdjacency, 3 * host.numTris,
                                       allocs);
            dev.triSampleAliasTable = devCopy(host.triSampleAliasTable,
                                              host.numTris, allocs);
            rawDealloc(host.vertices);
            rawDealloc(host.triIndices);
            rawDealloc(host.triAdjacency);
            rawDealloc(host.triSampleAliasTable);
        }
    }

    // the meshes as the device holds them
    for (uint32_t m = 0; m < num_meshes; m++) {
        const Navmesh &nav = navs[m];
        const uint32_t t0 = tri_offsets[m];
        if (nav.numTris != tri_offsets[m + 1] - t0 || nav.numTris > max_tris) {
            return cleanup(-5);
        }
        std::vector<Navmesh::AliasEntry> tbl(nav.numTris);
        (void)hipMemcpy(tri_idx + 3 * t0, nav.triIndices,
                        sizeof(uint32_t) * 3 * nav.numTris, hipMemcpyDeviceToHost);
        (void)hipMemcpy(adjacency + 3 * t0, nav.triAdjacency,
                        sizeof(uint32_t) * 3 * nav.numTris, hipMemcpyDeviceToHost);
        (void)hipMemcpy(tbl.data(), nav.triSampleAliasTable,
                        sizeof(Navmesh::AliasEntry) * nav.numTris,
                        hipMemcpyDeviceToHost);
        for (uint32_t i = 0; i < nav.numTris; i++) {
            tau[t0 + i] = tbl[i].tau;
            alias[t0 + i] = tbl[i].alias;
        }
        (void)hipMemcpy(out_verts + 3 * pms[m].vertOffset, nav.vertices,
                        sizeof(Vector3) * nav.numVerts, hipMemcpyDeviceToHost);
    }
    (void)total_tris;

    for (uint32_t q = 0; q < num_queries; q++) {
        if (query_mesh[q] >= num_meshes) {
            return cleanup(-6);
        }
    }

    const size_t per_query = (size_t)num_queries * max_tris;
    Navmesh *d_navs = devCopy(navs.data(), num_meshes, allocs);
    uint32_t *d_qmesh = devCopy(query_mesh, num_queries, allocs);
    RandKey *d_keys = devCopy((const RandKey *)keys, num_queries, allocs);
    QueryOut *d_out = devAlloc<QueryOut>(num_queries, allocs);
    uint32_t *d_bfs_order = devAlloc<uint32_t>(per_query, allocs);
    uint32_t *d_queue = devAlloc<uint32_t>(per_query, allocs);
    bool *d_visited = devAlloc<bool>(per_query, allocs);
    float *d_dist = devAlloc<float>(per_query, allocs);
    Vector3 *d_entries = devAlloc<Vector3>(per_query, allocs);
    uint32_t *d_heap = devAlloc<uint32_t>(per_query, allocs);
    uint32_t *d_heap_index = devAlloc<uint32_t>(per_query, allocs);
    uint32_t *d_pop_order = devAlloc<uint32_t>(per_query, allocs);
    float *d_pop_dist = devAlloc<float>(per_query, allocs);
    if (d_pop_dist == nullptr || d_pop_order == nullptr ||
            d_heap_index == nullptr || d_heap == nullptr ||
            d_entries == nullptr || d_dist == nullptr || d_visited == nullptr ||
            d_queue == nullptr || d_bfs_order == nullptr || d_out == nullptr ||
            d_keys == nullptr || d_qmesh == nullptr || d_navs == nullptr) {
        return cleanup(-2);
    }

    hipLaunchKernelGGL(queryKernel, dim3((num_queries + 63) / 64), dim3(64), 0,
                       0, d_navs, d_qmesh, d_keys, num_queries, max_tris,
                       radius2, d_out, d_bfs_order, d_queue, d_visited, d_dist,
                       d_entries, d_heap, d_heap_index, d_pop_order,
                       d_pop_dist);
    if (hipDeviceSynchronize() != hipSuccess) {
        return cleanup(-3);
    }
    (void)hipMemcpy(query_out, d_out, sizeof(QueryOut) * num_queries,
                    hipMemcpyDeviceToHost);
    (void)hipMemcpy(bfs_order, d_bfs_order, sizeof(uint32_t) * per_query,
                    hipMemcpyDeviceToHost);
    (void)hipMemcpy(pop_order, d_pop_order, sizeof(uint32_t) * per_query,
                    hipMemcpyDeviceToHost);
    (void)hipMemcpy(pop_dist, d_pop_dist, sizeof(float) * per_query,
                    hipMemcpyDeviceToHost);
    (void)hipMemcpy(distances, d_dist, sizeof(float) * per_query,
                    hipMemcpyDeviceToHost);
    (void)hipMemcpy(entries, d_entries, sizeof(Vector3) * per_query,
                    hipMemcpyDeviceToHost);
    return cleanup(0);
}

}
