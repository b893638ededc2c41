// TEST INFRASTRUCTURE.  Host compile of <madrona/navmesh.hpp> behind a C ABI
// for tests/test_navmesh_cpu.py: the builder, sampling, BFS and Dijkstra run
// on the CPU and are compared with the numpy restatement
// (tests/navmesh_restate.py) and the recorded fixture
// (tests/golden/navmesh_ref.npz).  Only the public Navmesh API is used, so the
// same file also compiles against the reference's headers.
//
// BFS accepts a polygon whose centroid (a + b + c) * (1/3) lies within
// sqrt(radius2) of the query's center, like navmesh_agents.  Dijkstra's
// entry points are zeroed before each search (the reference leaves entries of
// unreached polygons untouched).
#include <madrona/memory.hpp>
#include <madrona/navmesh.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace madrona;
using namespace madrona::math;

extern "C" {

#define API __attribute__((visibility("default")))

API void *nav_host_build(const float *verts, uint32_t num_verts,
                         const uint32_t *idxs, const uint32_t *offsets,
                         const uint32_t *sizes, uint32_t num_polys)
{
    std::vector<Vector3> v(num_verts);
    for (uint32_t i = 0; i < num_verts; i++) {
        v[i] = Vector3 { verts[3 * i], verts[3 * i + 1], verts[3 * i + 2] };
    }
    uint32_t num_idxs = 0;
    for (uint32_t i = 0; i < num_polys; i++) {
        num_idxs = std::max(num_idxs, offsets[i] + sizes[i]);
    }
    std::vector<uint32_t> i_copy(idxs, idxs + num_idxs);
    std::vector<uint32_t> o_copy(offsets, offsets + num_polys);
    std::vector<uint32_t> s_copy(sizes, sizes + num_polys);

    Navmesh *nav = new Navmesh(Navmesh::initFromPolygons(v.data(),
        i_copy.data(), o_copy.data(), s_copy.data(), num_verts, num_polys));
    return nav;
}

API void nav_host_free(void *h)
{
    Navmesh *nav = (Navmesh *)h;
    rawDealloc(nav->vertices);
    rawDealloc(nav->triIndices);
    rawDealloc(nav->triAdjacency);
    rawDealloc(nav->triSampleAliasTable);
    delete nav;
}

API uint32_t nav_host_num_tris(void *h)
{
    return ((Navmesh *)h)->numTris;
}

// tri_idx / adjacency: 3 per triangle; tau / alias: 1 per triangle;
// vertices: 3 floats per vertex
API void nav_host_read(void *h, uint32_t *tri_idx, uint32_t *adjacency,
                       float *tau, uint32_t *alias, float *vertices)
{
    Navmesh *nav = (Navmesh *)h;
    memcpy(tri_idx, nav->triIndices, sizeof(uint32_t) * 3 * nav->numTris);
    memcpy(adjacency, nav->triAdjacency, sizeof(uint32_t) * 3 * nav->numTris);
    for (uint32_t i = 0; i < nav->numTris; i++) {
        tau[i] = nav->triSampleAliasTable[i].tau;
        alias[i] = nav->triSampleAliasTable[i].alias;
    }
    memcpy(vertices, nav->vertices, sizeof(Vector3) * nav->numVerts);
}

// keys: (a, b) per query
API void nav_host_sample(void *h, const uint32_t *keys, uint32_t n,
                         float *points, uint32_t *polys)
{
    Navmesh *nav = (Navmesh *)h;
    for (uint32_t q = 0; q < n; q++) {
        Vector3 p = nav->samplePointAndPoly(RandKey { keys[2 * q], keys[2 * q + 1] },
                                            &polys[q]);
        points[3 * q] = p.x;
        points[3 * q + 1] = p.y;
        points[3 * q + 2] = p.z;
    }
}

// orders: numTris per query (visit order, count entries valid)
API void nav_host_bfs(void *h, const uint32_t *starts, const float *centers,
                      float radius2, uint32_t n, uint32_t *orders,
                      uint32_t *counts)
{
    Navmesh *nav = (Navmesh *)h;
    const uint32_t T = nav->numTris;
    std::vector<uint32_t> queue(T);
    bool *visited = (bool *)malloc(T + 1);
    for (uint32_t q = 0; q < n; q++) {
        Vector3 center { centers[3 * q], centers[3 * q + 1], centers[3 * q + 2] };
        uint32_t *order = orders + (size_t)q * T;
        uint32_t count = 0;
        nav->bfsFromPoly(starts[q], Navmesh::BFSState { queue.data(), visited },
            [&](uint32_t poly) {
                order[count++] = poly;
                Vector3 a, b, c;
                nav->getTriangleVertices(poly, &a, &b, &c);
                Vector3 centroid = (a + b + c) * (1.f / 3.f);
                return (centroid - center).length2() <= radius2;
            });
        counts[q] = count;
    }
    free(visited);
}

// distances, orders, pop_dists: numTris per query; entries: 3 * numTris
API void nav_host_dijkstra(void *h, const uint32_t *starts,
                           const float *start_pos, uint32_t n,
                           float *distances, float *entries, uint32_t *orders,
                           float *pop_dists, uint32_t *counts)
{
    Navmesh *nav = (Navmesh *)h;
    const uint32_t T = nav->numTris;
    std::vector<uint32_t> heap(T), heap_index(T);
    for (uint32_t q = 0; q < n; q++) {
        float *dist = distances + (size_t)q * T;
        Vector3 *entry = (Vector3 *)(entries + (size_t)q * 3 * T);
        memset(entry, 0, sizeof(Vector3) * T);
        uint32_t *order = orders + (size_t)q * T;
        float *pop_dist = pop_dists + (size_t)q * T;
        uint32_t count = 0;
        Vector3 pos { start_pos[3 * q], start_pos[3 * q + 1], start_pos[3 * q + 2] };
        nav->dijkstrasFromPoly(starts[q], pos,
            Navmesh::DijkstrasState { dist, entry, heap.data(), heap_index.data() },
            [&](uint32_t poly, Vector3, float d) {
                order[count] = poly;
                pop_dist[count] = d;
                count++;
            });
        counts[q] = count;
    }
}

}
