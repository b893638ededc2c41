// The four "models" of sims/render_prep, which sims/raycast_probe draws too.
#pragma once

#include "mesh_set.hpp"

namespace simmesh {

// of the ten materials below, the one no mesh here uses and raycast_probe's
// sheared cube takes
inline constexpr int32_t kDemoGrey = 4;

// Triangle meshes of the four "models": a cube, an ellipsoid (168 triangles: a
// bottom-level BVH several levels deep), a flat cylinder and a wedge.
// Materials: one per object for the first three; the wedge's mesh has none of
// its own (-1): its triangles carry theirs -- a textured one (a checker,
// sampled at the hit's interpolated uv) on the floor and the slope, a plain one
// on the sides, none on the back; a fifth material is only ever reached through
// MaterialOverride, a sixth (textured) too.
static inline MeshSet demoMeshes()
{
    MeshSet m;
    const int32_t red = m.material(0.8f, 0.2f, 0.2f);
    const int32_t green = m.material(0.2f, 0.7f, 0.3f);
    const int32_t blue = m.material(0.25f, 0.35f, 0.9f);
    m.material(0.9f, 0.8f, 0.1f);
    m.material(0.5f, 0.5f, 0.5f);           // kDemoGrey
    const int32_t checker = m.checkerTexture(16, 8, 2);
    const int32_t stripes = m.checkerTexture(5, 7, 1);
    const int32_t tiled = m.material(1.f, 0.9f, 0.8f, checker);
    const int32_t plain = m.material(0.3f, 0.8f, 0.8f);
    m.material(0.7f, 1.f, 0.6f, stripes);

    m.box(-0.5f, -0.5f, -0.5f, 0.5f, 0.5f, 0.5f);
    m.endObject(red);
    m.ellipsoid(0.f, 0.f, 1.f, 1.f, 0.25f, 1.f, 12, 8);
    m.endObject(green);
    m.cylinder(0.75f, -0.1f, 0.1f, 16);
    m.endObject(blue);
    // wedge in [0, 1.5] x [0, 1] x [0, 0.5]
    // (uvs run past [0, 1]: wrap addressing)
    m.vert(0.f, 0.f, 0.f); m.uv(0.f, 0.f);
    m.vert(1.5f, 0.f, 0.f); m.uv(1.5f, 0.f);
    m.vert(0.f, 1.f, 0.f); m.uv(0.f, 1.f);
    m.vert(1.5f, 1.f, 0.f); m.uv(1.5f, 1.f);
    m.vert(0.f, 0.f, 0.5f); m.uv(-0.25f, 0.1f);
    m.vert(0.f, 1.f, 0.5f); m.uv(-0.25f, 0.9f);
    m.currentTriangleMaterial = tiled;
    m.quad(0, 2, 3, 1);         // floor
    m.currentTriangleMaterial = -1;
    m.quad(0, 4, 5, 2);         // back
    m.currentTriangleMaterial = tiled;
    m.quad(1, 3, 5, 4);         // slope
    m.currentTriangleMaterial = plain;
    m.tri(0, 1, 4); m.tri(2, 5, 3);
    m.currentTriangleMaterial = -1;
    m.endObject(-1);
    return m;
}

}
