// The polygon sets navmesh_agents builds its worlds' navmeshes from.  Plain
// functions over caller buffers: the device TU runs them in the world
// constructors, the manager exports them to the tests (sim_navmesh_polygons in
// mgr.cpp), and both produce the same bits (integer RNG, fp32 + and * only,
// -ffp-contract=off).
//
// Families (flags & 7: 0 = per world, (global_world + seed) % 5; k = family k-1):
//   0  7 x 7 grid of unit quads with holes; every fifth cell a pentagon with a
//      vertex in the middle of its bottom edge (an exactly zero-area fan
//      triangle).  Integer coordinates: many exactly equal path lengths.
//   1  5 x 5 jittered grid; cells are fans of 5- to 8-gons (a vertex near the
//      middle of the bottom edge always, of the other edges at random)
//   2  two 3 x 3 quad grids ten units apart (disconnected islands)
//   3  4 x 4 quad grid with two fin triangles standing on one interior edge
//      (four triangles share that edge)
//   4  a single triangle
#pragma once

#include <madrona/math.hpp>
#include <madrona/rand.hpp>

namespace navmesh_agents {

inline constexpr uint32_t kNumFamilies = 5;
inline constexpr uint32_t kMaxVerts = 128;
inline constexpr uint32_t kMaxPolyIdxs = 256;
inline constexpr uint32_t kMaxPolys = 64;
inline constexpr uint32_t kWorkWords = 64;

struct PolygonSet {
    madrona::math::Vector3 *verts;      // [kMaxVerts]
    uint32_t *idxs;                     // [kMaxPolyIdxs]
    uint32_t *offsets;                  // [kMaxPolys]
    uint32_t *sizes;                    // [kMaxPolys]
    uint32_t *work;                     // [kWorkWords] (the generator's own)
    uint32_t numVerts;
    uint32_t numIdxs;
    uint32_t numPolys;
};

inline uint32_t meshFamily(uint32_t global_world, uint32_t seed,
                           uint32_t flags)
{
    uint32_t f = flags & 7u;
    if (f == 0 || f > kNumFamilies) {
        return (global_world + seed) % kNumFamilies;
    }
    return f - 1;
}

namespace detail {

inline uint32_t addVert(PolygonSet &out, float x, float y, float z)
{
    out.verts[out.numVerts] = madrona::math::Vector3 { x, y, z };
    return out.numVerts++;
}

inline void beginPoly(PolygonSet &out)
{
    out.offsets[out.numPolys] = out.numIdxs;
    out.sizes[out.numPolys] = 0;
}

inline void polyIdx(PolygonSet &out, uint32_t v)
{
    out.idxs[out.numIdxs++] = v;
    out.sizes[out.numPolys]++;
}

inline void endPoly(PolygonSet &out)
{
    out.numPolys++;
}

// (n + 1)^2 grid vertices at integer coordinates, offset by x0
inline uint32_t gridVerts(PolygonSet &out, uint32_t n, float x0)
{
    uint32_t base = out.numVerts;
    for (uint32_t y = 0; y <= n; y++) {
        for (uint32_t x = 0; x <= n; x++) {
            addVert(out, x0 + (float)x, (float)y, 0.f);
        }
    }
    return base;
}

inline void quad(PolygonSet &out, uint32_t base, uint32_t n, uint32_t cx,
                 uint32_t cy)
{
    uint32_t row = n + 1;
    beginPoly(out);
    polyIdx(out, base + cy * row + cx);
    polyIdx(out, base + cy * row + cx + 1);
    polyIdx(out, base + (cy + 1) * row + cx + 1);
    polyIdx(out, base + (cy + 1) * row + cx);
    endPoly(out);
}

inline float jitter(madrona::RandKey k, uint32_t i, float scale)
{
    return (madrona::rand::sampleUniform(madrona::rand::split_i(k, i)) - 0.5f) *
        scale;
}

inline void gridWithHoles(PolygonSet &out, madrona::RandKey key)
{
    constexpr uint32_t n = 7;
    uint32_t base = gridVerts(out, n, 0.f);
    uint32_t row = n + 1;
    for (uint32_t cy = 0; cy < n; cy++) {
        for (uint32_t cx = 0; cx < n; cx++) {
            uint32_t cell = cy * n + cx;
            // about one cell in six is a hole (never the first one)
            if (cell != 0 && madrona::rand::sampleI32(
                    madrona::rand::split_i(key, cell), 0, 6) == 0) {
                continue;
            }
            if (cell % 5 != 0) {
                quad(out, base, n, cx, cy);
                continue;
            }
            uint32_t mid = addVert(out, (float)cx + 0.5f, (float)cy, 0.f);
            beginPoly(out);
            polyIdx(out, base + cy * row + cx);
            polyIdx(out, mid);
            polyIdx(out, base + cy * row + cx + 1);
            polyIdx(out, base + (cy + 1) * row + cx + 1);
            polyIdx(out, base + (cy + 1) * row + cx);
            endPoly(out);
        }
    }
}

inline void jitteredFans(PolygonSet &out, madrona::RandKey key)
{
    constexpr uint32_t n = 5;
    constexpr uint32_t row = n + 1;
    madrona::RandKey corner_key = madrona::rand::split_i(key, 0);
    madrona::RandKey mid_key = madrona::rand::split_i(key, 1);

    for (uint32_t y = 0; y <= n; y++) {
        for (uint32_t x = 0; x <= n; x++) {
            uint32_t i = y * row + x;
            addVert(out, (float)x * 1.5f + jitter(corner_key, 3 * i, 0.5f),
                    (float)y * 1.5f + jitter(corner_key, 3 * i + 1, 0.5f),
                    jitter(corner_key, 3 * i + 2, 0.2f));
        }
    }

    // midpoint vertex of each grid edge, or ~0u: horizontal edges (x, y) ->
    // (x + 1, y) first, n * (n + 1) of them, then vertical ones (x, y) ->
    // (x, y + 1).  Edges that are some cell's bottom edge always have one.
    // (caller memory: a private array indexed at run time would be scratch)
    uint32_t *h_mid = out.work;
    uint32_t *v_mid = out.work + n * row;
    auto midpoint = [&](uint32_t a, uint32_t b, uint32_t j) {
        madrona::math::Vector3 m = (out.verts[a] + out.verts[b]) * 0.5f;
        return addVert(out, m.x + jitter(mid_key, 3 * j, 0.2f),
                       m.y + jitter(mid_key, 3 * j + 1, 0.2f),
                       m.z + jitter(mid_key, 3 * j + 2, 0.1f));
    };
    for (uint32_t y = 0; y <= n; y++) {
        for (uint32_t x = 0; x < n; x++) {
            uint32_t e = y * n + x;
            bool has = y < n || madrona::rand::sampleBool(
                madrona::rand::split_i(mid_key, 1000 + e));
            h_mid[e] = has ? midpoint(y * row + x, y * row + x + 1, e) : ~0u;
        }
    }
    for (uint32_t y = 0; y < n; y++) {
        for (uint32_t x = 0; x <= n; x++) {
            uint32_t e = y * row + x;
            bool has = madrona::rand::sampleBool(
                madrona::rand::split_i(mid_key, 2000 + e));
            v_mid[e] = has ? midpoint(y * row + x, (y + 1) * row + x,
                                      n * row + e) : ~0u;
        }
    }

    for (uint32_t cy = 0; cy < n; cy++) {
        for (uint32_t cx = 0; cx < n; cx++) {
            uint32_t c00 = cy * row + cx;
            uint32_t c10 = c00 + 1;
            uint32_t c11 = c10 + row;
            uint32_t c01 = c00 + row;
            uint32_t bottom = h_mid[cy * n + cx];
            uint32_t right = v_mid[cy * row + cx + 1];
            uint32_t top = h_mid[(cy + 1) * n + cx];
            uint32_t left = v_mid[cy * row + cx];

            beginPoly(out);
            polyIdx(out, c00);
            polyIdx(out, bottom);
            polyIdx(out, c10);
            if (right != ~0u) polyIdx(out, right);
            polyIdx(out, c11);
            if (top != ~0u) polyIdx(out, top);
            polyIdx(out, c01);
            if (left != ~0u) polyIdx(out, left);
            endPoly(out);
        }
    }
}

inline void twoIslands(PolygonSet &out)
{
    constexpr uint32_t n = 3;
    for (uint32_t island = 0; island < 2; island++) {
        uint32_t base = gridVerts(out, n, island == 0 ? 0.f : 10.f);
        for (uint32_t cy = 0; cy < n; cy++) {
            for (uint32_t cx = 0; cx < n; cx++) {
                quad(out, base, n, cx, cy);
            }
        }
    }
}

inline void gridWithFins(PolygonSet &out)
{
    constexpr uint32_t n = 4;
    uint32_t base = gridVerts(out, n, 0.f);
    for (uint32_t cy = 0; cy < n; cy++) {
        for (uint32_t cx = 0; cx < n; cx++) {
            quad(out, base, n, cx, cy);
        }
    }
    // the edge (2, 1) -- (2, 2) between cells (1, 1) and (2, 1)
    uint32_t row = n + 1;
    uint32_t p = base + 1 * row + 2;
    uint32_t q = base + 2 * row + 2;
    uint32_t up = addVert(out, 2.f, 1.5f, 1.f);
    uint32_t down = addVert(out, 2.f, 1.5f, -1.25f);
    beginPoly(out);
    polyIdx(out, p);
    polyIdx(out, q);
    polyIdx(out, up);
    endPoly(out);
    beginPoly(out);
    polyIdx(out, q);
    polyIdx(out, p);
    polyIdx(out, down);
    endPoly(out);
}

inline void singleTriangle(PolygonSet &out)
{
    uint32_t a = addVert(out, 0.f, 0.f, 0.f);
    uint32_t b = addVert(out, 2.f, 0.f, 0.f);
    uint32_t c = addVert(out, 0.f, 1.5f, 0.f);
    beginPoly(out);
    polyIdx(out, a);
    polyIdx(out, b);
    polyIdx(out, c);
    endPoly(out);
}

}

// Fills `out` (whose counts are reset) with one family's polygons; `key`
// drives the holes and the jitter.
inline void generatePolygons(uint32_t family, madrona::RandKey key,
                             PolygonSet &out)
{
    out.numVerts = 0;
    out.numIdxs = 0;
    out.numPolys = 0;
    switch (family) {
    case 0: detail::gridWithHoles(out, key); break;
    case 1: detail::jitteredFans(out, key); break;
    case 2: detail::twoIslands(out); break;
    case 3: detail::gridWithFins(out); break;
    default: detail::singleTriangle(out); break;
    }
}

}
