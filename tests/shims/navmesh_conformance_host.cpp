// TEST INFRASTRUCTURE.  Host half of the navmesh API conformance check (see
// navmesh_conformance.hip): the same members named from plain host C++, and
// the struct layout of the reference's navmesh.hpp reported for the test.
#include <madrona/navmesh.hpp>

#include <cstddef>

using namespace madrona;

extern "C" {

#define API __attribute__((visibility("default")))

// out[16]: sizeof / offsetof of Navmesh, AliasEntry, PathFindQueue, BFSState,
// DijkstrasState, and the sentinel
API void navconf_layout(uint64_t *out)
{
    out[0] = sizeof(Navmesh);
    out[1] = offsetof(Navmesh, vertices);
    out[2] = offsetof(Navmesh, triIndices);
    out[3] = offsetof(Navmesh, triAdjacency);
    out[4] = offsetof(Navmesh, triSampleAliasTable);
    out[5] = offsetof(Navmesh, numVerts);
    out[6] = offsetof(Navmesh, numTris);
    out[7] = sizeof(Navmesh::AliasEntry);
    out[8] = offsetof(Navmesh::AliasEntry, alias);
    out[9] = offsetof(Navmesh::PathFindQueue, heapSize);
    out[10] = sizeof(Navmesh::BFSState);
    out[11] = offsetof(Navmesh::BFSState, visited);
    out[12] = sizeof(Navmesh::DijkstrasState);
    out[13] = offsetof(Navmesh::DijkstrasState, entryPoints);
    out[14] = offsetof(Navmesh::DijkstrasState, heapIndex);
    out[15] = Navmesh::sentinel;
}

// A unit square as one quad, through the host API: returns numTris * 100 +
// the number of polygons Dijkstra pops from triangle 0 (2 * 100 + 2)
API uint32_t navconf_square()
{
    math::Vector3 verts[4] = {
        { 0.f, 0.f, 0.f }, { 1.f, 0.f, 0.f }, { 1.f, 1.f, 0.f }, { 0.f, 1.f, 0.f },
    };
    uint32_t idxs[4] = { 0, 1, 2, 3 };
    uint32_t offsets[1] = { 0 };
    uint32_t sizes[1] = { 4 };
    Navmesh nav = Navmesh::initFromPolygons(verts, idxs, offsets, sizes, 4, 1);

    float dist[2];
    math::Vector3 entries[2];
    uint32_t heap[2], heap_index[2];
    uint32_t pops = 0;
    nav.dijkstrasFromPoly(0, nav.samplePoint(rand::initKey(1)),
        Navmesh::DijkstrasState { dist, entries, heap, heap_index },
        [&](uint32_t, math::Vector3, float) { pops++; });

    uint32_t queue[2];
    bool visited[2];
    uint32_t visits = 0;
    nav.bfsFromPoly(1, Navmesh::BFSState { queue, visited },
                    [&](uint32_t) { visits++; return true; });

    uint32_t result = nav.numTris * 100 + pops + 10 * (visits - 2);
    rawDealloc(nav.vertices);
    rawDealloc(nav.triIndices);
    rawDealloc(nav.triAdjacency);
    rawDealloc(nav.triSampleAliasTable);
    return result;
}

}
