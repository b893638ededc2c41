// Navmesh definitions (see navmesh.hpp).  Line references are to the
// reference's include/madrona/navmesh.inl (queries) and src/common/navmesh.cpp
// (heap, builder).
//
// Device code: the queries keep every small array in registers (the three
// edge midpoints are selected by an unrolled loop index); all
// search state is caller memory, as in the reference.
//
// Memory of initFromPolygons:
//   host    rawAlloc (malloc) per array, like the reference: vertices, indices,
//           adjacency and alias table are the caller's to rawDealloc; the
//           temporaries are freed before returning.
//   device  one lane per world (world constructor).  The four outputs are ONE
//           persistent-region block (rawAlloc -> mwhip::persistAlloc, a bump
//           allocator never handed back), each array 128-B aligned:
//           navmesh_detail::deviceBlockBytes.  The temporaries (edge hash table,
//           weights, alias stacks) are ONE block of the executor's scratch
//           region (mwGPU::TmpAllocator, ecs_state::tmpBase): the executor
//           rewinds that region before every constructor pass and after the
//           last one, so they cost the persistent region nothing.  Every
//           output and temporary element is written before it is read, so a
//           second constructor pass builds the same mesh.
//           When an allocation of the pass did not fit (either region;
//           mwGPU::allocOverflowed), the builder reads and writes nothing and
//           returns an empty mesh (numTris 0): the overflowed allocation is the
//           region's base, other lanes' memory.  The executor then sizes both
//           regions from what the pass asked for and runs the constructors
//           again (constructWorlds).
#pragma once

namespace madrona {

namespace navmesh_detail {

// reference navmesh.cpp:9-17
MADRONA_HD inline CountT heapParent(CountT idx)
{
    return (idx - 1) / 2;
}

MADRONA_HD inline CountT heapChildOffset(CountT idx)
{
    return 2 * idx + 1;
}

// reference navmesh.cpp:19-41
MADRONA_HD inline void heapMoveUp(CountT moved_idx,
                                  uint32_t moved_poly,
                                  float moved_cost,
                                  uint32_t *heap,
                                  uint32_t *heap_index,
                                  float *costs)
{
    while (moved_idx != 0) {
        CountT parent_idx = heapParent(moved_idx);
        uint32_t parent_poly = heap[parent_idx];
        if (costs[parent_poly] <= moved_cost) {
            break;
        }

        heap[moved_idx] = parent_poly;
        heap_index[parent_poly] = (uint32_t)moved_idx;

        moved_idx = parent_idx;
    }

    heap[moved_idx] = moved_poly;
    heap_index[moved_poly] = (uint32_t)moved_idx;
}

// MurmurHash2 finalizer over an edge's two vertex ids (reference
// navmesh.cpp:105-121)
MADRONA_HD inline uint32_t hashEdge(uint32_t a, uint32_t b)
{
    const uint32_t m = 0x5bd1e995;

    a ^= b >> 18;
    a *= m;
    b ^= a >> 22;
    b *= m;
    a ^= b >> 17;
    a *= m;
    b ^= a >> 19;
    b *= m;

    return b;
}

// open-addressing slot of the builder's edge table (reference
// navmesh.cpp:240-245)
struct EdgeEntry {
    uint32_t vertA;
    uint32_t vertB;
    uint32_t firstTriIdx;
    uint32_t firstTriEdgeOffset;
};

MADRONA_HD constexpr inline uint64_t align128(uint64_t v)
{
    return (v + 127ull) & ~127ull;
}

// Byte offsets of the device builder's output block: vertices, triangle
// indices, adjacency, alias table, each 128-B aligned from the block's start.
struct DeviceBlockLayout {
    uint64_t indices;
    uint64_t adjacency;
    uint64_t aliasTable;
    uint64_t total;
};

MADRONA_HD constexpr inline DeviceBlockLayout deviceBlockLayout(
    uint32_t num_verts, uint32_t num_tris)
{
    DeviceBlockLayout l {};
    l.indices = align128((uint64_t)num_verts * sizeof(math::Vector3));
    l.adjacency = l.indices + align128((uint64_t)num_tris * 3 * sizeof(uint32_t));
    l.aliasTable = l.adjacency +
        align128((uint64_t)num_tris * 3 * sizeof(uint32_t));
    l.total = l.aliasTable +
        (uint64_t)num_tris * sizeof(Navmesh::AliasEntry);
    return l;
}

// What one device initFromPolygons takes from the persistent region: the
// block, plus the slack that lets its start be aligned to 128 B inside a
// 16-B granule allocation (mwhip::persistAlloc rounds to 16 B).
MADRONA_HD constexpr inline uint64_t deviceBlockBytes(uint32_t num_verts,
                                                      uint32_t num_tris)
{
    return (deviceBlockLayout(num_verts, num_tris).total + 112ull + 15ull) &
        ~15ull;
}

// ... and from the scratch region: edge table (3T), weights (T), alias
// stacks (2T)
MADRONA_HD constexpr inline uint64_t deviceTmpBytes(uint32_t num_tris)
{
    return (uint64_t)num_tris * 3 * sizeof(EdgeEntry) +
        (uint64_t)num_tris * sizeof(float) +
        (uint64_t)num_tris * 2 * sizeof(uint32_t);
}

// The builder proper (reference navmesh.cpp:123-316) over memory the caller
// provides; `out_vertices` already holds the copied vertices.
MADRONA_HD inline void buildNavmesh(const math::Vector3 *poly_vertices,
                                    const uint32_t *poly_idxs,
                                    const uint32_t *poly_idx_offsets,
                                    const uint32_t *poly_sizes,
                                    uint32_t num_polys,
                                    uint32_t num_tris,
                                    uint32_t *tri_indices,
                                    uint32_t *tri_adjacency,
                                    Navmesh::AliasEntry *alias_tbl,
                                    float *tri_weights,
                                    uint32_t *alias_stack,
                                    EdgeEntry *edge_tbl)
{
    using namespace math;
    constexpr uint32_t sentinel = Navmesh::sentinel;

    uint32_t *under_stack = alias_stack;
    uint32_t *over_stack = alias_stack + num_tris;
    uint32_t under_stack_size = 0;
    uint32_t over_stack_size = 0;

    // fan triangulation + twice the area of every triangle (:158-185)
    float tri_weight_sum = 0.f;
    uint32_t cur_tri = 0;
    for (CountT i = 0; i < (CountT)num_polys; i++) {
        uint32_t poly_size = poly_sizes[i];
        uint32_t poly_idx_base = poly_idx_offsets[i];
        for (uint32_t tri_offset = 1; tri_offset < poly_size - 1; tri_offset++) {
            uint32_t idx_a = poly_idxs[poly_idx_base];
            uint32_t idx_b = poly_idxs[poly_idx_base + tri_offset];
            uint32_t idx_c = poly_idxs[poly_idx_base + tri_offset + 1];

            tri_indices[3 * cur_tri] = idx_a;
            tri_indices[3 * cur_tri + 1] = idx_b;
            tri_indices[3 * cur_tri + 2] = idx_c;

            Vector3 a = poly_vertices[idx_a];
            Vector3 b = poly_vertices[idx_b];
            Vector3 c = poly_vertices[idx_c];

            Vector3 ab = b - a;
            Vector3 ac = c - a;
            float tri_area_x2 = cross(ab, ac).length();
            tri_weights[cur_tri] = tri_area_x2;
            tri_weight_sum += tri_area_x2;

            cur_tri++;
        }
    }

    // Vose's alias method, under / over stacks popped from the top (:187-235)
    for (uint32_t tri_idx = 0; tri_idx < num_tris; tri_idx++) {
        float normalized_weight =
            tri_weights[tri_idx] * float(num_tris) / tri_weight_sum;
        tri_weights[tri_idx] = normalized_weight;

        if (normalized_weight < 1.f) {
            under_stack[under_stack_size++] = tri_idx;
        } else {
            over_stack[over_stack_size++] = tri_idx;
        }
    }

    while (under_stack_size != 0 && over_stack_size != 0) {
        uint32_t under_idx = under_stack[--under_stack_size];
        uint32_t over_idx = over_stack[--over_stack_size];

        alias_tbl[under_idx] = Navmesh::AliasEntry {
            tri_weights[under_idx],
            over_idx,
        };

        float new_over_weight =
            (tri_weights[over_idx] + tri_weights[under_idx]) - 1.f;
        tri_weights[over_idx] = new_over_weight;

        if (new_over_weight < 1.f) {
            under_stack[under_stack_size++] = over_idx;
        } else {
            over_stack[over_stack_size++] = over_idx;
        }
    }

    for (uint32_t i = 0; i < under_stack_size; i++) {
        uint32_t idx = under_stack[i];
        alias_tbl[idx] = Navmesh::AliasEntry { 1.f, idx };
    }

    for (uint32_t i = 0; i < over_stack_size; i++) {
        uint32_t idx = over_stack[i];
        alias_tbl[idx] = Navmesh::AliasEntry { 1.f, idx };
    }

    // adjacency through an open-addressing edge table of 3T slots (:247-304).
    // An edge met a second time links the two triangles; a third triangle on
    // the same edge links to the first one again and takes over the first
    // one's side of that edge (the second keeps its link to the first).
    uint32_t max_edges = num_tris * 3;
    for (uint32_t i = 0; i < max_edges; i++) {
        tri_adjacency[i] = sentinel;
        edge_tbl[i] = EdgeEntry { sentinel, sentinel, sentinel, 0 };
    }

    auto recordEdge = [edge_tbl, tri_adjacency, max_edges](
        uint32_t tri_idx, uint32_t tri_edge_offset, uint32_t a, uint32_t b)
    {
        if (b < a) {
            uint32_t t = a;
            a = b;
            b = t;
        }

        // Lemire's multiply-shift in place of a modulo
        uint32_t edge_hash = utils::u32mulhi(hashEdge(a, b), max_edges);

        while (edge_tbl[edge_hash].vertA != sentinel && (
                edge_tbl[edge_hash].vertA != a ||
                edge_tbl[edge_hash].vertB != b)) {
            edge_hash = edge_hash == max_edges - 1 ? 0 : edge_hash + 1;
        }

        EdgeEntry &entry = edge_tbl[edge_hash];
        entry.vertA = a;
        entry.vertB = b;

        if (entry.firstTriIdx == sentinel) {
            entry.firstTriIdx = tri_idx;
            entry.firstTriEdgeOffset = tri_edge_offset;
        } else {
            uint32_t other_tri_idx = entry.firstTriIdx;
            uint32_t other_tri_edge_offset = entry.firstTriEdgeOffset;

            tri_adjacency[3 * tri_idx + tri_edge_offset] = other_tri_idx;
            tri_adjacency[3 * other_tri_idx + other_tri_edge_offset] = tri_idx;
        }
    };

    for (uint32_t tri_idx = 0; tri_idx < num_tris; tri_idx++) {
        uint32_t a_idx = tri_indices[3 * tri_idx];
        uint32_t b_idx = tri_indices[3 * tri_idx + 1];
        uint32_t c_idx = tri_indices[3 * tri_idx + 2];

        recordEdge(tri_idx, 0, a_idx, b_idx);
        recordEdge(tri_idx, 1, b_idx, c_idx);
        recordEdge(tri_idx, 2, c_idx, a_idx);
    }
}

}

// ---- PathFindQueue (reference navmesh.cpp:43-103) -----------------------------

MADRONA_HD void Navmesh::PathFindQueue::add(uint32_t poly, float cost)
{
    costs[poly] = cost;

    CountT new_idx = heapSize++;
    navmesh_detail::heapMoveUp(new_idx, poly, cost, heap, heapIndex, costs);
}

MADRONA_HD uint32_t Navmesh::PathFindQueue::removeMin()
{
    using navmesh_detail::heapChildOffset;

    uint32_t root_poly = heap[0];

    uint32_t moved_poly = heap[--heapSize];
    float moved_cost = costs[moved_poly];

    CountT moved_idx = 0;
    CountT child_offset;
    while ((child_offset = heapChildOffset(moved_idx)) < heapSize) {
        CountT child_idx = child_offset;
        uint32_t child_poly = heap[child_idx];
        float child_cost = costs[child_poly];

        // the cheaper child; the left one on a tie
        CountT right_idx = child_idx + 1;
        if (right_idx < heapSize) {
            uint32_t right_poly = heap[right_idx];
            float right_cost = costs[right_poly];
            if (right_cost < child_cost) {
                child_idx = right_idx;
                child_poly = right_poly;
                child_cost = right_cost;
            }
        }

        // strictly cheaper than that child: moved_poly stays here
        if (moved_cost < child_cost) {
            break;
        }

        heap[moved_idx] = child_poly;
        heapIndex[child_poly] = (uint32_t)moved_idx;

        moved_idx = child_idx;
    }

    heap[moved_idx] = moved_poly;
    heapIndex[moved_poly] = (uint32_t)moved_idx;

    heapIndex[root_poly] = Navmesh::sentinel;
    return root_poly;
}

MADRONA_HD void Navmesh::PathFindQueue::decreaseCost(uint32_t poly, float cost)
{
    costs[poly] = cost;

    CountT cur_idx = (CountT)heapIndex[poly];

    navmesh_detail::heapMoveUp(cur_idx, poly, cost, heap, heapIndex, costs);
}

// ---- queries (reference navmesh.inl) -------------------------------------------

// reference navmesh.inl:5-34 (samplePoint :36-40, getTriangleVertices :42-50)
MADRONA_HD math::Vector3 Navmesh::samplePointAndPoly(RandKey rnd,
                                                     uint32_t *out_poly)
{
    using namespace math;

    RandKey tbl_row_rnd = rand::split_i(rnd, 0);
    RandKey alias_p_rnd = rand::split_i(rnd, 1);
    RandKey bary_rnd = rand::split_i(rnd, 2);

    uint32_t tbl_row_idx = rand::sampleI32(tbl_row_rnd, 0, numTris);
    float p = rand::sampleUniform(alias_p_rnd);

    AliasEntry tbl_row = triSampleAliasTable[tbl_row_idx];

    uint32_t tri_idx = p < tbl_row.tau ? tbl_row_idx : tbl_row.alias;
    *out_poly = tri_idx;

    Vector3 a, b, c;
    getTriangleVertices(tri_idx, &a, &b, &c);

    Vector2 uv = rand::sample2xUniform(bary_rnd);

    if (uv.x + uv.y > 1.f) {
        uv.x = 1.f - uv.x;
        uv.y = 1.f - uv.y;
    }

    float w = 1.f - uv.x - uv.y;

    return a * uv.x + b * uv.y + c * w;
}

MADRONA_HD math::Vector3 Navmesh::samplePoint(RandKey rnd)
{
    uint32_t poly;
    return samplePointAndPoly(rnd, &poly);
}

MADRONA_HD void Navmesh::getTriangleVertices(uint32_t tri_idx,
                                             math::Vector3 *out_a,
                                             math::Vector3 *out_b,
                                             math::Vector3 *out_c)
{
    *out_a = vertices[triIndices[3 * tri_idx]];
    *out_b = vertices[triIndices[3 * tri_idx + 1]];
    *out_c = vertices[triIndices[3 * tri_idx + 2]];
}

// reference navmesh.inl:52-83
template <typename Fn>
MADRONA_HD void Navmesh::bfsFromPoly(uint32_t start_poly,
                                     BFSState bfs_state,
                                     Fn &&fn)
{
    ArrayQueue<uint32_t> bfs_queue(bfs_state.queue, numTris);
    bool *visited = bfs_state.visited;

    utils::zeroN<bool>(visited, numTris);

    bfs_queue.add(start_poly);
    visited[start_poly] = true;

    while (!bfs_queue.isEmpty()) {
        uint32_t poly = bfs_queue.remove();

        bool accept = fn(poly);
        if (!accept) {
            continue;
        }

        MADRONA_UNROLL
        for (CountT i = 0; i < 3; i++) {
            uint32_t adjacent = triAdjacency[3 * poly + i];

            if (adjacent != sentinel && !visited[adjacent]) {
                bfs_queue.add(adjacent);
                visited[adjacent] = true;
            }
        }
    }
}

// reference navmesh.inl:86-154
template <typename Fn>
MADRONA_HD void Navmesh::dijkstrasFromPoly(
    uint32_t start_poly,
    math::Vector3 start_pos,
    DijkstrasState dijkstras_state,
    Fn &&fn)
{
    using namespace math;

    float *distances = dijkstras_state.distances;

    PathFindQueue prio_queue {
        distances,
        dijkstras_state.heap,
        dijkstras_state.heapIndex,
        0,
    };
    utils::fillN<uint32_t>(prio_queue.heapIndex, sentinel, numTris);
    utils::fillN<float>(distances, FLT_MAX, numTris);

    Vector3 *entry_points = dijkstras_state.entryPoints;
    entry_points[start_poly] = start_pos;

    prio_queue.add(start_poly, 0.f);
    while (prio_queue.heapSize > 0) {
        uint32_t min_poly = prio_queue.removeMin();
        Vector3 cur_pos = entry_points[min_poly];
        float dist_so_far = distances[min_poly];

        fn(min_poly, cur_pos, dist_so_far);

        Vector3 a, b, c;
        getTriangleVertices(min_poly, &a, &b, &c);

        MADRONA_UNROLL
        for (CountT i = 0; i < 3; i++) {
            uint32_t adjacent = triAdjacency[3 * min_poly + i];
            if (adjacent == Navmesh::sentinel) {
                continue;
            }

            // edge i runs from vertex i to vertex i + 1 (the reference's
            // edge_midpoints[i]); a select of registers, never a private array
            Vector3 e0 = i == 0 ? a : (i == 1 ? b : c);
            Vector3 e1 = i == 0 ? b : (i == 1 ? c : a);
            Vector3 edge_midpoint = (e0 + e1) / 2.f;

            float dist_to_edge = cur_pos.distance(edge_midpoint);
            float new_dist = dist_so_far + dist_to_edge;
            float prev_dist = distances[adjacent];

            if (new_dist >= prev_dist) {
                continue;
            }

            entry_points[adjacent] = edge_midpoint;

            uint32_t prio_queue_idx = prio_queue.heapIndex[adjacent];
            if (prio_queue_idx == sentinel) {
                prio_queue.add(adjacent, new_dist);
            } else {
                prio_queue.decreaseCost(adjacent, new_dist);
            }
        }
    }
}

// reference navmesh.cpp:123-316
MADRONA_HD Navmesh Navmesh::initFromPolygons(
    math::Vector3 *poly_vertices,
    uint32_t *poly_idxs,
    uint32_t *poly_idx_offsets,
    uint32_t *poly_sizes,
    uint32_t num_verts,
    uint32_t num_polys)
{
    using namespace math;
    using navmesh_detail::EdgeEntry;

#if defined(__HIP_DEVICE_COMPILE__)
    // An allocation of this constructor pass did not fit (the caller's input
    // buffers may be among them, i.e. memory other lanes write): read and
    // write nothing, return an empty mesh.  The executor sizes the regions
    // and runs the constructors again.
    if (mwGPU::allocOverflowed()) {
        return Navmesh {};
    }
#endif

    uint32_t num_tris = 0;
    for (CountT i = 0; i < (CountT)num_polys; i++) {
        num_tris += poly_sizes[i] - 2;
    }

#if defined(__HIP_DEVICE_COMPILE__)
    const navmesh_detail::DeviceBlockLayout layout =
        navmesh_detail::deviceBlockLayout(num_verts, num_tris);
    char *block = (char *)rawAlloc(
        navmesh_detail::deviceBlockBytes(num_verts, num_tris));
    block = (char *)navmesh_detail::align128((uint64_t)(uintptr_t)block);

    Vector3 *out_vertices = (Vector3 *)block;
    uint32_t *tri_indices = (uint32_t *)(block + layout.indices);
    uint32_t *tri_adjacency = (uint32_t *)(block + layout.adjacency);
    AliasEntry *alias_tbl = (AliasEntry *)(block + layout.aliasTable);

    // temporaries: edge table first (16-B entries), then weights and stacks
    char *tmp = (char *)mwGPU::TmpAllocator::get().alloc(
        navmesh_detail::deviceTmpBytes(num_tris));
    EdgeEntry *edge_tbl = (EdgeEntry *)tmp;
    float *tri_weights = (float *)(edge_tbl + 3 * (uint64_t)num_tris);
    uint32_t *alias_stack = (uint32_t *)(tri_weights + num_tris);

    // either block did not fit: it is the region's base, shared with other
    // lanes (a lane always sees its own overflow)
    if (mwGPU::allocOverflowed()) {
        return Navmesh {};
    }
#else
    Vector3 *out_vertices = (Vector3 *)rawAlloc(sizeof(Vector3) * num_verts);
    uint32_t *tri_indices =
        (uint32_t *)rawAlloc(sizeof(uint32_t) * 3 * num_tris);
    uint32_t *tri_adjacency =
        (uint32_t *)rawAlloc(sizeof(uint32_t) * 3 * num_tris);
    AliasEntry *alias_tbl =
        (AliasEntry *)rawAlloc(sizeof(AliasEntry) * num_tris);

    float *tri_weights = (float *)rawAlloc(sizeof(float) * num_tris);
    uint32_t *alias_stack =
        (uint32_t *)rawAlloc(sizeof(uint32_t) * num_tris * 2);
    EdgeEntry *edge_tbl =
        (EdgeEntry *)rawAlloc(sizeof(EdgeEntry) * num_tris * 3);
#endif

    utils::copyN<Vector3>(out_vertices, poly_vertices, num_verts);

    navmesh_detail::buildNavmesh(poly_vertices, poly_idxs, poly_idx_offsets,
        poly_sizes, num_polys, num_tris, tri_indices, tri_adjacency, alias_tbl,
        tri_weights, alias_stack, edge_tbl);

#if !defined(__HIP_DEVICE_COMPILE__)
    rawDealloc(edge_tbl);
    rawDealloc(alias_stack);
    rawDealloc(tri_weights);
#endif

    return Navmesh {
        out_vertices,
        tri_indices,
        tri_adjacency,
        alias_tbl,
        num_verts,
        num_tris,
    };
}

}
