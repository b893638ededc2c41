#include "raycast_probe/sim.hpp"

#include "common/demo_meshes.hpp"
#include "common/render_mgr.hpp"
#ifndef SIM_BACKEND_REF_CPU
#include "common/render_config.hpp"
#endif

#include <vector>

namespace {

// flags: bit 1 = depth only, bit 3 = the geometry goes to the executor in the
// reference's asset form (MeshBVHData / MaterialData) instead of as plain
// triangles, bit 5 = kind 8 deeper than the ray caster's traversal stack,
// bits 8-15 = ray caster output resolution (HIP backend; 0 = ray caster off)
constexpr uint32_t kMaxRecordsPerWorld = 128;
simmgr::RenderMgr g_render;

// sims/render_prep's four meshes and ten materials (common/demo_meshes.hpp: a
// cube, a 168-triangle ellipsoid, a flat cylinder, a wedge whose triangles
// carry their own materials, two of them textured) and a fifth mesh: the cube sheared along x,
// twelve triangles that are NOT their own bounding box -- the ray caster walks
// its tree where it intersects the cube as slabs -- with uvs of its own.
const simmesh::MeshSet &meshes()
{
    static const simmesh::MeshSet set = [] {
        simmesh::MeshSet m = simmesh::demoMeshes();
        // the cube with x += z / 2
        {
            const size_t first = m.vertices.size() / 3;
            m.box(-0.5f, -0.5f, -0.5f, 0.5f, 0.5f, 0.5f);
            for (size_t v = first; v < m.vertices.size() / 3; v++) {
                const float y = m.vertices[3 * v + 1], z = m.vertices[3 * v + 2];
                m.vertices[3 * v] += 0.5f * z;
                m.vertexUVs[2 * v] = 0.75f + 1.5f * z;
                m.vertexUVs[2 * v + 1] = 0.5f + 0.8f * y + 0.3f * z;
            }
            m.endObject(simmesh::kDemoGrey);
        }
        return m;
    }();
    return set;
}

}

struct SimTraits {
    using Sim = raycastprobe::Sim;
    using Engine = raycastprobe::Engine;

    static constexpr uint32_t numExports =
        (uint32_t)raycastprobe::ExportID::NumExports;
    static constexpr uint32_t numTaskGraphs = 1;

    static Sim::Config makeConfig(const SimCreateArgs &args)
    {
        g_render = simmgr::RenderMgr(args, kMaxRecordsPerWorld,
                                     raycastprobe::consts::numViewers,
                                     raycastprobe::consts::maxInstances);
        return Sim::Config { args.world_base, (args.flags >> 5) & 1u,
                             g_render.bridge() };
    }

    static void makeInits(const SimCreateArgs &, Sim::WorldInit *) {}

    static const simmesh::MeshSet &renderMeshes() { return meshes(); }

    static void preStep() { g_render.beginStep(); }

#ifndef SIM_BACKEND_REF_CPU
    static madrona::Optional<madrona::CudaBatchRenderConfig> renderConfig(
        const SimCreateArgs &args)
    {
        madrona::CudaBatchRenderConfig cfg {};
        g_render.readRenderFlags(cfg, args.flags, 1, 8, 0);
        // object-space root boxes of the meshes
        cfg.objectRootAABBs = madrona::Span<const float>(
            meshes().rootAABBs.data(),
            (madrona::CountT)(raycastprobe::consts::numObjects * 6));
        if ((args.flags & 8u) != 0u) {
            // (kept alive with the process: the executor copies what it needs
            // while it is constructed)
            simmgr::meshesToReferenceAssets(meshes(), cfg);
        } else {
            simmgr::meshesToRenderConfig(meshes(), cfg);
        }
        return madrona::Optional<madrona::CudaBatchRenderConfig>::make(cfg);
    }
#endif

    template <typename T>
    static void describeTensors(T &out, uint32_t num_worlds);
    template <typename T>
    static void describeColumns(T &cols);
};

#include "common/mgr_impl.inl"

template <typename T>
void SimTraits::describeTensors(T &out, uint32_t num_worlds)
{
    out.push_back({ "steps", SIM_I32, { (int64_t)num_worlds, 1 },
                    (uint32_t)raycastprobe::ExportID::Steps });
    // (two viewers per world)
    g_render.describeTensors(out, (int64_t)num_worlds * raycastprobe::consts::numViewers,
                             (uint32_t)raycastprobe::ExportID::RGB,
                             (uint32_t)raycastprobe::ExportID::Depth);
}

template <typename T>
void SimTraits::describeColumns(T &cols)
{
    using namespace raycastprobe;
    using namespace madrona::render;

    cols.template add<Thing, Position>("Thing.Position", true);
    cols.template add<LightArchetype, LightDesc>("Light.LightDesc", false);
    cols.template add<RenderableArchetype, MortonCode>("Renderable.MortonCode", false);
#ifndef SIM_BACKEND_REF_CPU
    // GPU mode only: the render entities' rows ARE the renderer's records (the
    // reference's CPU mode appends them to the bridge: render_prep_bridge_records)
    cols.template add<RenderableArchetype, InstanceData>("Renderable.InstanceData", false);
    cols.template add<RenderCameraArchetype, PerspectiveCameraData>("Camera.PerspectiveCameraData", false);
#endif
}

SIM_RENDER_BRIDGE_RECORDS(g_render)
