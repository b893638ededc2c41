#include "tgs_drop/sim.hpp"

#include "common/rigid_body_set.hpp"

#include <vector>
#include <string>

namespace {

using namespace madrona;
using namespace madrona::phys;
using simmgr::HullSource;

// object 0: a unit cube; object 1: a slab (2 x 1 x 0.5) with three different
// principal moments, so that the gyroscopic term of the integrator is not zero
ObjectManager *loadObjects(const SimCreateArgs &args)
{
    simmgr::RigidBodySet set(2);
    const uint32_t cube = set.addHull(HullSource::box(-0.5f, 0.5f));
    const uint32_t slab = set.addHull(
        HullSource::box({ -1.f, -0.5f, -0.25f }, { 1.f, 0.5f, 0.25f }));
    set.hull(0, cube, 1.f, { 0.5f, 0.5f });
    set.hull(1, slab, 0.4f, { 0.5f, 0.5f });
    return set.load(args, 4);
}

}

struct SimTraits {
    using Sim = tgsdrop::Sim;
    using Engine = tgsdrop::Engine;

    static constexpr uint32_t numExports = (uint32_t)tgsdrop::ExportID::NumExports;
    static constexpr uint32_t numTaskGraphs = 1;

    static Sim::Config makeConfig(const SimCreateArgs &args)
    {
        return Sim::Config { args.seed, args.world_base, loadObjects(args) };
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
    out.push_back({ "step_count", SIM_I32, { (int64_t)num_worlds, 1 },
                    (uint32_t)tgsdrop::ExportID::StepCount });
}

template <typename T>
void SimTraits::describeColumns(T &cols)
{
    using namespace tgsdrop;
    using madrona::Entity;
    using namespace madrona::phys;

    cols.template add<Body, Entity>("Body.Entity", false);
    cols.template add<Body, Position>("Body.Position", true);
    cols.template add<Body, Rotation>("Body.Rotation", true);
    cols.template add<Body, Velocity>("Body.Velocity", true);
    cols.template add<Body, ExternalForce>("Body.ExternalForce", true);
    cols.template add<Body, ExternalTorque>("Body.ExternalTorque", true);
    cols.template add<Body, broadphase::LeafID>("Body.LeafID", false);
    cols.template add<Anchor, Entity>("Anchor.Entity", false);
    cols.template add<Anchor, Position>("Anchor.Position", true);
    cols.template add<Anchor, Velocity>("Anchor.Velocity", true);
}
