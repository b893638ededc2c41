#include "escape_room_phys/sim.hpp"

#include "common/rigid_body_set.hpp"
#ifdef ESCPHYS_RENDER
#include "common/mesh_set.hpp"
#include "common/render_mgr.hpp"
#ifndef SIM_BACKEND_REF_CPU
#include "common/render_config.hpp"
#endif
#endif

#include <vector>
#include <string>

namespace {

using namespace madrona;
using namespace madrona::phys;
using escphys::SimObject;

// A unit cube hull stands in for every mesh asset of the real Escape Room (no
// file importers here): instances scale it per body.
ObjectManager *loadPhysicsObjects(const SimCreateArgs &args)
{
    simmgr::RigidBodySet set((size_t)SimObject::NumObjects);
    const uint32_t cube = set.addHull(simmgr::HullSource::box(-0.5f, 0.5f));

    set.hull(SimObject::Cube, cube, 0.075f, { 0.5f, 0.75f });
    set.hull(SimObject::Wall, cube, 0.f, { 0.5f, 0.5f });
    set.hull(SimObject::Door, cube, 0.f, { 0.5f, 0.5f });
    set.hull(SimObject::Agent, cube, 1.f, { 0.5f, 0.5f });
    set.hull(SimObject::Button, cube, 1.f, { 0.5f, 0.5f });
    set.plane(SimObject::Plane);

    return set.load(args, 10, simmgr::turnAboutZOnly(SimObject::Agent));
}

#ifdef ESCPHYS_RENDER
// What the ray caster draws for each SimObject: boxes for the cube-hull bodies
// (instances scale them), a 352-triangle ellipsoid for the agents, a quad for
// the floor.
const simmesh::MeshSet &meshes()
{
    static const simmesh::MeshSet set = [] {
        simmesh::MeshSet m;
        const int32_t cube = m.material(0.8f, 0.45f, 0.2f);
        const int32_t wall = m.material(0.55f, 0.55f, 0.6f);
        const int32_t door = m.material(0.2f, 0.6f, 0.25f);
        const int32_t agent = m.material(0.9f, 0.85f, 0.2f);
        const int32_t button = m.material(0.85f, 0.15f, 0.15f);
        const int32_t floor = m.material(0.35f, 0.3f, 0.28f);
        const int32_t mats[] = { cube, wall, door, agent, button, floor };
        for (int32_t obj = 0; obj < (int32_t)SimObject::NumObjects; obj++) {
            if (obj == (int32_t)SimObject::Agent) {
                m.ellipsoid(0.f, 0.f, 0.f, 0.5f, 0.5f, 0.5f, 16, 12);
            } else if (obj == (int32_t)SimObject::Plane) {
                const uint32_t a = m.vert(-40.f, -20.f, 0.f);
                m.vert(40.f, -20.f, 0.f);
                m.vert(40.f, 60.f, 0.f);
                m.vert(-40.f, 60.f, 0.f);
                m.quad(a, a + 1, a + 2, a + 3);
            } else {
                m.box(-0.5f, -0.5f, -0.5f, 0.5f, 0.5f, 0.5f);
            }
            m.endObject(mats[obj]);
        }
        return m;
    }();
    return set;
}

// floor + 4 borders + 2 agents + 3 rooms x 9 = 34 instances, 2 views per world
constexpr uint32_t kMaxRecordsPerWorld = 64;
simmgr::RenderMgr g_render;
#endif

}

struct SimTraits {
    using Sim = escphys::Sim;
    using Engine = escphys::Engine;

    static constexpr uint32_t numExports =
        (uint32_t)escphys::ExportID::NumExports;
    static constexpr uint32_t numTaskGraphs = 1;

    // flags: low 16 bits = autoResetDenom (0 disables random resets); render
    // variant: bits 16-23 = output resolution (0: 64), bit 24 = depth only,
    // bit 25 = the sun casts shadows, bit 26 = no ray caster (render-prep
    // systems only: without render-target entities the entity ids are the CPU
    // backend's, whose CPU mode has no ray caster either)
    static Sim::Config makeConfig(const SimCreateArgs &args)
    {
#ifdef ESCPHYS_RENDER
        g_render = simmgr::RenderMgr(args, kMaxRecordsPerWorld,
                                     escphys::consts::numAgents,
                                     kMaxRecordsPerWorld);
#endif
        return Sim::Config {
            args.seed, args.world_base, args.flags & 0xFFFFu,
            loadPhysicsObjects(args),
#ifdef ESCPHYS_RENDER
            (args.flags >> 25) & 1u,
            g_render.bridge(),
#endif
        };
    }

#ifdef ESCPHYS_RENDER
    static void preStep() { g_render.beginStep(); }

    static const simmesh::MeshSet &renderMeshes() { return meshes(); }

#ifndef SIM_BACKEND_REF_CPU
    static madrona::Optional<madrona::CudaBatchRenderConfig> renderConfig(
        const SimCreateArgs &args)
    {
        if (((args.flags >> 26) & 1u) != 0u) {
            return madrona::Optional<madrona::CudaBatchRenderConfig>::none();
        }
        madrona::CudaBatchRenderConfig cfg {};
        g_render.readRenderFlags(cfg, args.flags, 24, 16, 64);
        cfg.maxViewsPerWorld = escphys::consts::numAgents;
        simmgr::meshesToRenderConfig(meshes(), cfg);
        return madrona::Optional<madrona::CudaBatchRenderConfig>::make(cfg);
    }
#endif
#endif

    static void makeInits(const SimCreateArgs &, Sim::WorldInit *) {}

    template <typename T>
    static void describeTensors(T &out, uint32_t num_worlds);
    template <typename T>
    static void describeColumns(T &cols);
};

#include "common/mgr_impl.inl"

template <typename T>
void SimTraits::describeTensors(T &out, uint32_t num_worlds)
{
    using escphys::ExportID;
    namespace c = escphys::consts;
    int64_t W = num_worlds;
    int64_t A = c::numAgents;
    out.push_back({ "reset", SIM_I32, { W, 1 }, (uint32_t)ExportID::Reset });
    out.push_back({ "action", SIM_I32, { W, A, 4 }, (uint32_t)ExportID::Action });
    out.push_back({ "reward", SIM_F32, { W, A, 1 }, (uint32_t)ExportID::Reward });
    out.push_back({ "done", SIM_I32, { W, A, 1 }, (uint32_t)ExportID::Done });
    out.push_back({ "self_obs", SIM_F32, { W, A, 8 },
                    (uint32_t)ExportID::SelfObservation });
    out.push_back({ "partner_obs", SIM_F32, { W, A, 3 },
                    (uint32_t)ExportID::PartnerObservation });
    out.push_back({ "room_ent_obs", SIM_F32,
                    { W, A, c::numCubesPerRoom + c::numButtonsPerRoom + 1, 3 },
                    (uint32_t)ExportID::RoomEntityObservations });
    out.push_back({ "door_obs", SIM_F32, { W, A, 3 },
                    (uint32_t)ExportID::DoorObservation });
    out.push_back({ "lidar", SIM_F32, { W, A, c::numLidarSamples, 2 },
                    (uint32_t)ExportID::Lidar });
    out.push_back({ "steps_remaining", SIM_I32, { W, A, 1 },
                    (uint32_t)ExportID::StepsRemaining });
#ifdef ESCPHYS_RENDER
    g_render.describeTensors(out, W * A, (uint32_t)ExportID::RGB,
                             (uint32_t)ExportID::Depth);
#endif
}

template <typename T>
void SimTraits::describeColumns(T &cols)
{
    using namespace escphys;
    using madrona::Entity;
    using madrona::phys::broadphase::LeafID;

    cols.template add<Agent, Entity>("Agent.Entity", false);
    cols.template add<Agent, Position>("Agent.Position", true);
    cols.template add<Agent, Rotation>("Agent.Rotation", true);
    cols.template add<Agent, Velocity>("Agent.Velocity", true);
    cols.template add<Agent, LeafID>("Agent.LeafID", false);
    cols.template add<Agent, ExternalForce>("Agent.ExternalForce", true);
    cols.template add<Agent, Action>("Agent.Action", false);
    cols.template add<Agent, Reward>("Agent.Reward", true);
    cols.template add<Agent, Done>("Agent.Done", false);
    cols.template add<Agent, SelfObservation>("Agent.SelfObservation", true);
    cols.template add<Agent, PartnerObservation>("Agent.PartnerObservation", true);
    cols.template add<Agent, RoomEntityObservations>(
        "Agent.RoomEntityObservations", true);
    cols.template add<Agent, DoorObservation>("Agent.DoorObservation", true);
    cols.template add<Agent, Lidar>("Agent.Lidar", true);
    cols.template add<Agent, StepsRemaining>("Agent.StepsRemaining", false);
    cols.template add<Agent, Progress>("Agent.Progress", true);
    cols.template add<Agent, GrabState>("Agent.GrabState", false);

    cols.template add<PhysicsEntity, Entity>("PhysicsEntity.Entity", false);
    cols.template add<PhysicsEntity, Position>("PhysicsEntity.Position", true);
    cols.template add<PhysicsEntity, Rotation>("PhysicsEntity.Rotation", true);
    cols.template add<PhysicsEntity, Velocity>("PhysicsEntity.Velocity", true);
    cols.template add<PhysicsEntity, LeafID>("PhysicsEntity.LeafID", false);
    cols.template add<PhysicsEntity, EntityType>("PhysicsEntity.EntityType", false);

    cols.template add<DoorEntity, Entity>("DoorEntity.Entity", false);
    cols.template add<DoorEntity, Position>("DoorEntity.Position", true);
    cols.template add<DoorEntity, OpenState>("DoorEntity.OpenState", false);
    cols.template add<DoorEntity, DoorProperties>("DoorEntity.DoorProperties", false);

    cols.template add<ButtonEntity, Entity>("ButtonEntity.Entity", false);
    cols.template add<ButtonEntity, Position>("ButtonEntity.Position", true);
    cols.template add<ButtonEntity, ButtonState>("ButtonEntity.ButtonState", false);
#ifdef ESCPHYS_RENDER
    using namespace madrona::render;
    // the light table is filled the same way on both backends
    cols.template add<LightArchetype, LightDesc>("Light.LightDesc", false);
    cols.template add<PhysicsEntity, Renderable>("PhysicsEntity.Renderable", false);
    cols.template add<ButtonEntity, Renderable>("ButtonEntity.Renderable", false);
    cols.template add<Agent, Renderable>("Agent.Renderable", false);
    cols.template add<Agent, RenderCamera>("Agent.RenderCamera", false);
#ifndef SIM_BACKEND_REF_CPU
    // GPU mode only: the render entities' rows ARE the renderer's records
    cols.template add<RenderableArchetype, InstanceData>("Renderable.InstanceData", false);
    cols.template add<RenderableArchetype, MortonCode>("Renderable.MortonCode", false);
    cols.template add<RenderCameraArchetype, PerspectiveCameraData>("Camera.PerspectiveCameraData", false);
    cols.template add<RenderCameraArchetype, RenderOutputIndex>("Camera.RenderOutputIndex", false);
#endif
#endif
}

#ifdef ESCPHYS_RENDER
SIM_RENDER_BRIDGE_RECORDS(g_render)
#endif
