#include "render_prep/sim.hpp"

#include "common/demo_meshes.hpp"
#include "common/render_mgr.hpp"
#ifndef SIM_BACKEND_REF_CPU
#include "common/render_config.hpp"
#endif

#include <vector>

namespace {

// flags: bit 4 = movers stand on a coarse grid (Morton-code ties);
// bit 0 = RenderingSystem::setupTasks(update_visual_properties = true),
// bit 1 = depth only, bit 2 = crowded worlds, bit 3 = the geometry goes to the
// executor in the reference's asset form (MeshBVHData / MaterialData) instead
// of as plain triangles,
// bits 8-15 = ray caster output resolution (HIP backend; 0 = ray caster off)
constexpr uint32_t kMaxRecordsPerWorld = 128;
simmgr::RenderMgr g_render;

// object-space root boxes of the four "models" (HIP backend, ray caster on)
const float kRootAABBs[renderprep::consts::numObjects * 6] = {
    -0.5f, -0.5f, -0.5f, 0.5f, 0.5f, 0.5f,
    -1.f, -0.25f, 0.f, 1.f, 0.25f, 2.f,
    -0.75f, -0.75f, -0.1f, 0.75f, 0.75f, 0.1f,
    0.f, 0.f, 0.f, 1.5f, 1.f, 0.5f,
};

// their triangle meshes, inside those boxes
const simmesh::MeshSet &meshes()
{
    static const simmesh::MeshSet set = simmesh::demoMeshes();
    return set;
}

}

struct SimTraits {
    using Sim = renderprep::Sim;
    using Engine = renderprep::Engine;

    static constexpr uint32_t numExports =
        (uint32_t)renderprep::ExportID::NumExports;
    static constexpr uint32_t numTaskGraphs = 1;

    static Sim::Config makeConfig(const SimCreateArgs &args)
    {
        g_render = simmgr::RenderMgr(args, kMaxRecordsPerWorld,
                                     renderprep::consts::numViewers,
                                     renderprep::consts::maxMovers);
        return Sim::Config { args.seed, args.world_base, args.flags & 1u,
                             (args.flags >> 2) & 1u, (args.flags >> 4) & 1u,
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
        cfg.objectRootAABBs = madrona::Span<const float>(
            kRootAABBs, (madrona::CountT)(renderprep::consts::numObjects * 6));
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
    out.push_back({ "roster", SIM_I32, { (int64_t)num_worlds, 2 },
                    (uint32_t)renderprep::ExportID::Roster });
    // (two viewers per world)
    g_render.describeTensors(out, (int64_t)num_worlds * renderprep::consts::numViewers,
                             (uint32_t)renderprep::ExportID::RGB,
                             (uint32_t)renderprep::ExportID::Depth);
}

template <typename T>
void SimTraits::describeColumns(T &cols)
{
    using namespace renderprep;
    using namespace madrona::render;

    // simulator side: identical rows in identical order on both backends
    cols.template add<Mover, Position>("Mover.Position", true);
    cols.template add<Mover, Rotation>("Mover.Rotation", true);
    cols.template add<Mover, Renderable>("Mover.Renderable", false);
    cols.template add<Mover, MaterialOverride>("Mover.MaterialOverride", false);
    cols.template add<Mover, ColorOverride>("Mover.ColorOverride", false);
    cols.template add<Viewer, Position>("Viewer.Position", true);
    cols.template add<Lamp, Position>("Lamp.Position", true);
    // render side.  The light table is filled the same way on both backends;
    // Morton codes too, but the reference's CPU sort by Morton code is not a
    // sort: compared per world as multisets.
    cols.template add<LightArchetype, LightDesc>("Light.LightDesc", false);
    cols.template add<RenderableArchetype, MortonCode>("Renderable.MortonCode", false);
#ifndef SIM_BACKEND_REF_CPU
    // GPU mode only: the render entities' rows ARE the renderer's records
    cols.template add<RenderableArchetype, madrona::Entity>("Renderable.Entity", false);
    cols.template add<RenderableArchetype, InstanceData>("Renderable.InstanceData", false);
    cols.template add<RenderableArchetype, TLBVHNode>("Renderable.TLBVHNode", true);
    cols.template add<RenderCameraArchetype, PerspectiveCameraData>("Camera.PerspectiveCameraData", false);
    cols.template add<RenderCameraArchetype, RenderOutputIndex>("Camera.RenderOutputIndex", false);
    cols.template add<RenderCameraArchetype, RenderOutputRef>("Camera.RenderOutputRef", false);
#endif
}

SIM_RENDER_BRIDGE_RECORDS(g_render)
