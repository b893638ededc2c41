#include "hideseek/sim.hpp"

#include "common/rigid_body_set.hpp"

#include <vector>
#include <string>

namespace {

using namespace madrona;
using namespace madrona::phys;
using hideseek::SimObject;
using simmgr::HullSource;

ObjectManager *loadPhysicsObjects(const SimCreateArgs &args)
{
    simmgr::RigidBodySet set((size_t)SimObject::NumObjects);

    // two unit hulls, scaled per instance
    const uint32_t cube = set.addHull(HullSource::box(-0.5f, 0.5f));
    const uint32_t wedge = set.addHull(HullSource::wedge());
    // the L-shaped block: a bar along x and a post standing on one end
    const uint32_t bar = set.addHull(
        HullSource::box({ -1.f, -0.3f, -0.5f }, { 1.f, 0.3f, 0.1f }));
    const uint32_t post = set.addHull(
        HullSource::box({ 0.4f, -0.3f, 0.1f }, { 1.f, 0.3f, 0.9f }));

    set.hull(SimObject::Box, cube, 0.1f, { 0.5f, 0.75f });
    set.hull(SimObject::LongBox, cube, 0.06f, { 0.5f, 0.75f });
    set.hull(SimObject::Ramp, wedge, 0.05f, { 0.6f, 0.8f });
    set.hull(SimObject::Wall, cube, 0.f, { 0.5f, 0.5f });
    set.hull(SimObject::Agent, cube, 1.f, { 0.5f, 0.5f });
    set.compound(SimObject::LBlock, { bar, post }, 0.08f, { 0.5f, 0.75f });
    set.plane(SimObject::Plane);

    return set.load(args, 10, simmgr::turnAboutZOnly(SimObject::Agent));
}

}

struct SimTraits {
    using Sim = hideseek::Sim;
    using Engine = hideseek::Engine;

    static constexpr uint32_t numExports =
        (uint32_t)hideseek::ExportID::NumExports;
    static constexpr uint32_t numTaskGraphs = 1;

    // flags: low 16 bits = autoResetDenom (0 disables random resets)
    static Sim::Config makeConfig(const SimCreateArgs &args)
    {
        return Sim::Config {
            args.seed, args.world_base, args.flags & 0xFFFFu,
            loadPhysicsObjects(args),
        };
    }

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
    using hideseek::ExportID;
    namespace c = hideseek::consts;
    int64_t W = num_worlds;
    int64_t A = c::numAgents;
    out.push_back({ "reset", SIM_I32, { W, 1 }, (uint32_t)ExportID::Reset });
    out.push_back({ "action", SIM_I32, { W, A, 4 }, (uint32_t)ExportID::Action });
    out.push_back({ "reward", SIM_F32, { W, A, 1 }, (uint32_t)ExportID::Reward });
    out.push_back({ "done", SIM_I32, { W, A, 1 }, (uint32_t)ExportID::Done });
    out.push_back({ "self_obs", SIM_F32, { W, A, 8 },
                    (uint32_t)ExportID::SelfObservation });
    out.push_back({ "agent_obs", SIM_F32, { W, A, A - 1, 4 },
                    (uint32_t)ExportID::AgentObservations });
    out.push_back({ "box_obs", SIM_F32, { W, A, c::numBoxes, 5 },
                    (uint32_t)ExportID::BoxObservations });
    out.push_back({ "ramp_obs", SIM_F32, { W, A, c::numRamps, 5 },
                    (uint32_t)ExportID::RampObservations });
    out.push_back({ "lidar", SIM_F32, { W, A, c::numLidarSamples, 2 },
                    (uint32_t)ExportID::Lidar });
    out.push_back({ "steps_remaining", SIM_I32, { W, A, 1 },
                    (uint32_t)ExportID::StepsRemaining });
}

template <typename T>
void SimTraits::describeColumns(T &cols)
{
    using namespace hideseek;
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
    cols.template add<Agent, AgentObservations>("Agent.AgentObservations", true);
    cols.template add<Agent, BoxObservations>("Agent.BoxObservations", true);
    cols.template add<Agent, RampObservations>("Agent.RampObservations", true);
    cols.template add<Agent, Lidar>("Agent.Lidar", true);
    cols.template add<Agent, StepsRemaining>("Agent.StepsRemaining", false);
    cols.template add<Agent, Visibility>("Agent.Visibility", false);

    cols.template add<MovableObject, Entity>("MovableObject.Entity", false);
    cols.template add<MovableObject, Position>("MovableObject.Position", true);
    cols.template add<MovableObject, Rotation>("MovableObject.Rotation", true);
    cols.template add<MovableObject, Velocity>("MovableObject.Velocity", true);
    cols.template add<MovableObject, ResponseType>(
        "MovableObject.ResponseType", false);
    cols.template add<MovableObject, LeafID>("MovableObject.LeafID", false);
    cols.template add<MovableObject, LockState>("MovableObject.LockState", false);

    cols.template add<StaticObject, Entity>("StaticObject.Entity", false);
    cols.template add<StaticObject, Position>("StaticObject.Position", true);
    cols.template add<StaticObject, Scale>("StaticObject.Scale", true);
    cols.template add<StaticObject, LeafID>("StaticObject.LeafID", false);
}
