// TEST INFRASTRUCTURE.  API conformance of <madrona/navmesh.hpp> and the
// utils.hpp pieces it rests on (ArrayQueue, copyN / zeroN / fillN), device
// side: a translation unit wrapped like a simulator's (user prelude, then the
// force_cuda_host_device pragma) whose kernel names every member a simulator
// may name.  A missing or mis-declared one fails the build; the host half is
// navmesh_conformance_host.cpp, the test tests/test_navmesh_cpu.py.
#include <madrona/mwhip/user_prelude.hpp>
#pragma clang force_cuda_host_device begin
#include <madrona/navmesh.hpp>
#include <madrona/utils.hpp>

using namespace madrona;
using namespace madrona::math;

namespace navconf {

inline uint32_t touchNavmesh(Navmesh &nav, RandKey key, char *scratch)
{
    uint32_t poly = 0;
    Vector3 p = nav.samplePointAndPoly(key, &poly);
    Vector3 q = nav.samplePoint(key);
    Vector3 a, b, c;
    nav.getTriangleVertices(poly, &a, &b, &c);

    uint32_t *u32 = (uint32_t *)scratch;
    const uint32_t T = nav.numTris;
    Navmesh::BFSState bfs { u32, (bool *)(u32 + T) };
    uint32_t visits = 0;
    nav.bfsFromPoly(poly, bfs, [&](uint32_t) { return ++visits < 4; });

    Navmesh::DijkstrasState dij {
        (float *)(u32 + 2 * T), (Vector3 *)(u32 + 3 * T), u32 + 6 * T,
        u32 + 7 * T,
    };
    float last = 0.f;
    nav.dijkstrasFromPoly(poly, p, dij, [&](uint32_t, Vector3, float d) {
        last = d;
    });

    Navmesh::PathFindQueue pq { dij.distances, dij.heap, dij.heapIndex, 0 };
    pq.add(0, 1.f);
    pq.decreaseCost(0, 0.5f);
    uint32_t min_poly = pq.removeMin();

    Navmesh::AliasEntry e = nav.triSampleAliasTable[0];
    ArrayQueue<uint32_t> aq(u32, 4);
    aq.add(e.alias);
    uint32_t r = aq.remove();
    aq.clear();
    utils::copyN<uint32_t>(u32, u32 + T, 1);
    utils::zeroN<uint32_t>(u32, 1);
    utils::fillN<uint32_t>(u32, Navmesh::sentinel, 1);

    return visits + min_poly + r + aq.capacity() + (aq.isEmpty() ? 1u : 0u) +
        (uint32_t)(last + q.x + a.x + b.y + c.z + e.tau) + nav.numVerts +
        (uint32_t)(uintptr_t)nav.vertices + (uint32_t)(uintptr_t)nav.triIndices +
        (uint32_t)(uintptr_t)nav.triAdjacency;
}

}
#pragma clang force_cuda_host_device end

__global__ void navConformanceKernel(Vector3 *verts, uint32_t *idxs,
                                     uint32_t *offsets, uint32_t *sizes,
                                     char *scratch, uint32_t *out)
{
    Navmesh nav = Navmesh::initFromPolygons(verts, idxs, offsets, sizes, 4, 1);
    out[threadIdx.x] = navconf::touchNavmesh(nav, rand::initKey(threadIdx.x),
                                             scratch);
}
