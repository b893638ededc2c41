// Triangle navmesh: area-weighted point sampling, BFS and Dijkstra over the
// triangles' edge adjacency.  API contract and struct layout: reference
// include/madrona/navmesh.hpp (whole file); the queries follow navmesh.inl,
// the builder and the search heap src/common/navmesh.cpp, operation for
// operation, so results equal the reference's bit for bit under
// -ffp-contract=off.
//
// The reference defines PathFindQueue's methods and initFromPolygons out of
// line in navmesh.cpp; here everything is inline MADRONA_HD (navmesh.inl):
// device code has no second translation unit to link against.  Where the
// builder's memory comes from on each side: navmesh.inl, INTEGRATION.md.
#pragma once

#include <madrona/math.hpp>
#include <madrona/memory.hpp>
#include <madrona/rand.hpp>
#include <madrona/utils.hpp>

#include <cfloat>
#include <cstdint>

namespace madrona {

struct Navmesh {
    // Binary min-heap over polygon ids keyed by costs[poly]; heapIndex[poly] is
    // the polygon's heap slot, or sentinel once popped / never pushed.
    struct PathFindQueue {
        float *costs;
        uint32_t *heap;
        uint32_t *heapIndex;
        CountT heapSize;

        MADRONA_HD inline void add(uint32_t poly, float cost);
        MADRONA_HD inline uint32_t removeMin();
        MADRONA_HD inline void decreaseCost(uint32_t poly, float cost);
    };

    // Vose alias table row: keep the row with probability tau, else alias
    struct AliasEntry {
        float tau;
        uint32_t alias;
    };

    math::Vector3 *vertices;
    uint32_t *triIndices;
    uint32_t *triAdjacency;
    AliasEntry *triSampleAliasTable;
    uint32_t numVerts;
    uint32_t numTris;

    MADRONA_HD inline math::Vector3 samplePointAndPoly(RandKey rnd,
                                                       uint32_t *out_poly);
    MADRONA_HD inline math::Vector3 samplePoint(RandKey rnd);

    MADRONA_HD inline void getTriangleVertices(uint32_t tri_idx,
                                               math::Vector3 *out_a,
                                               math::Vector3 *out_b,
                                               math::Vector3 *out_c);

    // caller memory, numTris entries each
    struct BFSState {
        uint32_t *queue;
        bool *visited;
    };

    // fn(poly) -> bool: false stops the search from expanding past poly
    template <typename Fn>
    MADRONA_HD inline void bfsFromPoly(
        uint32_t poly,
        BFSState bfs_state,
        Fn &&fn);

    // caller memory, numTris entries each
    struct DijkstrasState {
        float *distances;
        math::Vector3 *entryPoints;
        uint32_t *heap;
        uint32_t *heapIndex;
    };

    // fn(poly, entry_point, distance) for every polygon in pop order
    template <typename Fn>
    MADRONA_HD inline void dijkstrasFromPoly(
        uint32_t start_poly,
        math::Vector3 start_pos,
        DijkstrasState dijkstras_state,
        Fn &&fn);

    // Fan-triangulates the polygons (poly_sizes[i] >= 3 vertices starting at
    // poly_idxs[poly_idx_offsets[i]]), builds the alias table and adjacency.
    // The inputs are read only; the vertices are copied.
    MADRONA_HD static inline Navmesh initFromPolygons(
        math::Vector3 *poly_vertices,
        uint32_t *poly_idxs,
        uint32_t *poly_idx_offsets,
        uint32_t *poly_sizes,
        uint32_t num_verts,
        uint32_t num_polys);

    static constexpr inline uint32_t sentinel = 0xFFFF'FFFF;
};

}

#include "navmesh.inl"
