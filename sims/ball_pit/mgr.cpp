#include "ball_pit/sim.hpp"

#include "common/rigid_body_set.hpp"

#include <vector>
#include <string>

namespace {

using namespace madrona;
using namespace madrona::phys;
using ballpit::SimObject;
using simmgr::HullSource;

ObjectManager *loadPhysicsObjects(const SimCreateArgs &args)
{
    simmgr::RigidBodySet set((size_t)SimObject::NumObjects);

    // two unit hulls, scaled per instance
    const uint32_t cube = set.addHull(HullSource::box(-0.5f, 0.5f));
    set.addHull(HullSource::wedge());
    // the L-shaped block: a bar along x and a post standing on one end
    const uint32_t bar = set.addHull(
        HullSource::box({ -1.f, -0.3f, -0.3f }, { 1.f, 0.3f, 0.3f }));
    const uint32_t post = set.addHull(
        HullSource::box({ 0.4f, -0.3f, 0.3f }, { 1.f, 0.3f, 1.2f }));
    const uint32_t coin12 = set.addHull(HullSource::prism(12, 0.9f, 0.5f));
    const uint32_t coin16 = set.addHull(HullSource::prism(16, 1.f, 0.5f));

    set.hull(SimObject::Box, cube, 0.2f, { 0.5f, 0.75f });
    set.hull(SimObject::Coin12, coin12, 0.3f, { 0.6f, 0.8f });
    set.hull(SimObject::Coin16, coin16, 0.25f, { 0.6f, 0.8f });
    set.hull(SimObject::Wall, cube, 0.f, { 0.5f, 0.5f });
    set.compound(SimObject::LBlock, { bar, post }, 0.2f, { 0.5f, 0.7f });
    set.sphere(SimObject::Sphere, 1.f, 0.25f, { 0.5f, 0.6f });
    set.plane(SimObject::Plane);

    return set.load(args, 10);
}

}

struct SimTraits {
    using Sim = ballpit::Sim;
    using Engine = ballpit::Engine;

    static constexpr uint32_t numExports =
        (uint32_t)ballpit::ExportID::NumExports;
    static constexpr uint32_t numTaskGraphs = 1;

    // flags: low 16 bits = autoResetDenom (0 disables random resets), bits
    // 16-23 = extra bodies per world (crowd mode), bit 24 = every other joint
    // is a hinge, bit 25 = checkEntityAABBOverlap steers the kicks, bit 26 = only
    // ONE world is crowded, the one whose global index is in bits 27-31
    static Sim::Config makeConfig(const SimCreateArgs &args)
    {
        return Sim::Config {
            args.seed, args.world_base, args.flags & 0xFFFFu,
            (args.flags >> 16) & 0xFFu,
            loadPhysicsObjects(args),
            (args.flags >> 24) & 1u,
            (args.flags >> 25) & 1u,
            ((args.flags >> 26) & 1u) != 0 ?
                (int32_t)((args.flags >> 27) & 31u) : -1,
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
    using ballpit::ExportID;
    int64_t W = num_worlds;
    out.push_back({ "reset", SIM_I32, { W, 1 }, (uint32_t)ExportID::Reset });
    out.push_back({ "steps_remaining", SIM_I32, { W, 1 },
                    (uint32_t)ExportID::StepsRemaining });
    out.push_back({ "query_probe", SIM_I32, { W, 2 },
                    (uint32_t)ExportID::QueryProbe });
}

template <typename T>
void SimTraits::describeColumns(T &cols)
{
    using namespace ballpit;
    using madrona::Entity;
    using madrona::phys::broadphase::LeafID;

    cols.template add<MovableObject, Entity>("MovableObject.Entity", false);
    cols.template add<MovableObject, Position>("MovableObject.Position", true);
    cols.template add<MovableObject, Rotation>("MovableObject.Rotation", true);
    cols.template add<MovableObject, Scale>("MovableObject.Scale", true);
    cols.template add<MovableObject, Velocity>("MovableObject.Velocity", true);
    cols.template add<MovableObject, ExternalForce>(
        "MovableObject.ExternalForce", true);
    cols.template add<MovableObject, LeafID>("MovableObject.LeafID", false);
    cols.template add<MovableObject, KickIndex>("MovableObject.KickIndex", false);

    cols.template add<StaticObject, Entity>("StaticObject.Entity", false);
    cols.template add<StaticObject, Position>("StaticObject.Position", true);
    cols.template add<StaticObject, LeafID>("StaticObject.LeafID", false);
}
