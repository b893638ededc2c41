// The static meshes of the mesh_cast simulator, generated deterministically on
// the host (+, -, *, /, sqrt only, so every build gets the same bytes), and
// their MeshBVHs.  Families 0-4 are the ones worlds use (world w: w % 5):
//   0  a single triangle
//   1  a box room seen from inside (12 triangles, inward winding)
//   2  a flat floor quad (zero z-extent)
//   3  a 16 x 16 height field (512 triangles, vertices on the integer grid)
//   4  an ellipsoid (cube sphere, 432 triangles) with per-triangle materials
//      and non-zero uvs
// and two more exist for the builder's tests:
//   5  two triangles
//   6  4097 triangles
// Triangles wind counter-clockwise seen from the side they face (the side
// traceRay hits: back faces are culled).
//
// The builder is this backend's header; it is included by path because the
// reference's include directory has no such file and the reference-CPU build
// of this simulator must get the identical tree (the header only uses names
// both header sets define).
#pragma once

#include "../madrona_amd/include/madrona/mesh_bvh_builder.hpp"

#include <vector>

namespace mesh_cast {

inline constexpr uint32_t kNumWorldFamilies = 5;
inline constexpr uint32_t kNumFamilies = 7;

struct MeshData {
    std::vector<madrona::math::Vector3> positions;
    std::vector<madrona::math::Vector2> uvs;            // empty: none
    std::vector<uint32_t> indices;
    std::vector<uint32_t> faceMaterials;                // empty: materialIDX
    uint32_t materialIDX = 0;

    uint32_t numTris() const { return (uint32_t)(indices.size() / 3); }

    void tri(uint32_t a, uint32_t b, uint32_t c)
    {
        indices.push_back(a);
        indices.push_back(b);
        indices.push_back(c);
    }

    // makes triangle t face `towards` (true) or away from (false) `point`
    void orient(uint32_t t, madrona::math::Vector3 point, bool towards)
    {
        using namespace madrona::math;
        Vector3 a = positions[indices[3 * t]];
        Vector3 b = positions[indices[3 * t + 1]];
        Vector3 c = positions[indices[3 * t + 2]];
        float side = dot(cross(b - a, c - a), point - a);
        if ((side > 0.f) != towards) {
            uint32_t tmp = indices[3 * t + 1];
            indices[3 * t + 1] = indices[3 * t + 2];
            indices[3 * t + 2] = tmp;
        }
    }
};

inline float heightAt(uint32_t i, uint32_t j)
{
    return 0.25f * (float)((i * 5 + j * 3 + (i * j) % 7) % 5);
}

// nx x ny cells of unit size centred on the origin, heights from heightAt
inline void gridMesh(MeshData &m, uint32_t nx, uint32_t ny)
{
    using namespace madrona::math;
    for (uint32_t j = 0; j <= ny; j++) {
        for (uint32_t i = 0; i <= nx; i++) {
            m.positions.push_back(Vector3 {
                (float)i - (float)(nx / 2), (float)j - (float)(ny / 2),
                heightAt(i, j) });
        }
    }
    for (uint32_t j = 0; j < ny; j++) {
        for (uint32_t i = 0; i < nx; i++) {
            uint32_t v00 = j * (nx + 1) + i, v10 = v00 + 1;
            uint32_t v01 = v00 + nx + 1, v11 = v01 + 1;
            m.tri(v00, v10, v11);
            m.tri(v00, v11, v01);
        }
    }
}

inline MeshData generateMesh(uint32_t family)
{
    using namespace madrona::math;
    MeshData m;

    switch (family) {
    case 0: {
        m.positions = { { -3.f, -3.f, 0.5f }, { 3.f, -3.f, 0.5f },
                        { 0.f, 3.f, 1.f } };
        m.tri(0, 1, 2);
        m.materialIDX = 3;
    } break;
    case 1: {
        for (uint32_t k = 0; k < 8; k++) {
            m.positions.push_back(Vector3 { (k & 1) ? 4.f : -4.f,
                (k & 2) ? 4.f : -4.f, (k & 4) ? 4.f : 0.f });
        }
        const uint32_t quads[6][4] = {
            { 0, 1, 3, 2 }, { 4, 5, 7, 6 }, { 0, 1, 5, 4 },
            { 2, 3, 7, 6 }, { 0, 2, 6, 4 }, { 1, 3, 7, 5 },
        };
        for (const auto &q : quads) {
            m.tri(q[0], q[1], q[2]);
            m.tri(q[0], q[2], q[3]);
        }
        for (uint32_t t = 0; t < m.numTris(); t++) {
            m.orient(t, Vector3 { 0.f, 0.f, 2.f }, true);
            m.faceMaterials.push_back(t / 2);
        }
    } break;
    case 2: {
        m.positions = { { -4.f, -4.f, 0.f }, { 4.f, -4.f, 0.f },
                        { 4.f, 4.f, 0.f }, { -4.f, 4.f, 0.f } };
        m.tri(0, 1, 2);
        m.tri(0, 2, 3);
        m.materialIDX = 1;
    } break;
    case 3: {
        gridMesh(m, 16, 16);
        m.materialIDX = 2;
    } break;
    case 4: {
        // a cube's faces as n x n grids, pushed onto the unit sphere, scaled
        const uint32_t n = 6;
        const Vector3 radii { 1.5f, 1.f, 0.8f };
        const Vector3 centre { 0.f, 0.f, 1.2f };
        for (uint32_t face = 0; face < 6; face++) {
            uint32_t base = (uint32_t)m.positions.size();
            for (uint32_t j = 0; j <= n; j++) {
                for (uint32_t i = 0; i <= n; i++) {
                    float u = 2.f * (float)i / (float)n - 1.f;
                    float v = 2.f * (float)j / (float)n - 1.f;
                    float w = face % 2 == 0 ? 1.f : -1.f;
                    Vector3 p = face / 2 == 0 ? Vector3 { w, u, v } :
                        (face / 2 == 1 ? Vector3 { v, w, u } :
                                         Vector3 { u, v, w });
                    float inv_len = 1.f / sqrtf(p.x * p.x + p.y * p.y +
                                                p.z * p.z);
                    Vector3 d { p.x * inv_len, p.y * inv_len, p.z * inv_len };
                    m.positions.push_back(Vector3 {
                        centre.x + radii.x * d.x, centre.y + radii.y * d.y,
                        centre.z + radii.z * d.z });
                    m.uvs.push_back(Vector2 { 0.5f + 0.25f * d.x,
                                              0.5f + 0.25f * d.y });
                }
            }
            for (uint32_t j = 0; j < n; j++) {
                for (uint32_t i = 0; i < n; i++) {
                    uint32_t v00 = base + j * (n + 1) + i, v10 = v00 + 1;
                    uint32_t v01 = v00 + n + 1, v11 = v01 + 1;
                    m.tri(v00, v10, v11);
                    m.tri(v00, v11, v01);
                }
            }
        }
        for (uint32_t t = 0; t < m.numTris(); t++) {
            m.orient(t, centre, false);
            m.faceMaterials.push_back((t * 7) % 5);
        }
    } break;
    case 5: {
        m.positions = { { -2.f, -2.f, 1.f }, { 2.f, -2.f, 1.f },
                        { 2.f, 2.f, 1.5f }, { -2.f, 2.f, 1.25f } };
        m.tri(0, 1, 2);
        m.tri(0, 2, 3);
    } break;
    default: {
        gridMesh(m, 64, 32);
        uint32_t base = (uint32_t)m.positions.size();
        m.positions.push_back(Vector3 { 0.f, 0.f, 3.f });
        m.positions.push_back(Vector3 { 1.f, 0.f, 3.f });
        m.positions.push_back(Vector3 { 0.f, 1.f, 3.f });
        m.tri(base, base + 1, base + 2);
    } break;
    }

    return m;
}

inline madrona::MeshBVH buildMesh(MeshData &m)
{
    madrona::imp::SourceMesh src {};
    src.positions = m.positions.data();
    src.uvs = m.uvs.empty() ? nullptr : m.uvs.data();
    src.indices = m.indices.data();
    src.faceCounts = nullptr;
    src.faceMaterials = m.faceMaterials.empty() ? nullptr :
        m.faceMaterials.data();
    src.numVertices = (uint32_t)m.positions.size();
    src.numFaces = m.numTris();
    src.materialIDX = m.materialIDX;
    return madrona::MeshBVHBuilder::build(
        madrona::Span<const madrona::imp::SourceMesh>(&src, 1));
}

// the host trees of all families, built on first use
struct FamilyTrees {
    MeshData data[kNumFamilies];
    madrona::MeshBVH bvh[kNumFamilies];

    FamilyTrees()
    {
        for (uint32_t f = 0; f < kNumFamilies; f++) {
            data[f] = generateMesh(f);
            bvh[f] = buildMesh(data[f]);
        }
    }

    ~FamilyTrees()
    {
        for (madrona::MeshBVH &b : bvh) {
            madrona::MeshBVHBuilder::free(b);
        }
    }
};

inline FamilyTrees &familyTrees()
{
    static FamilyTrees trees;
    return trees;
}

}
