#include "contact_probe/sim.hpp"

#include "common/rigid_body_set.hpp"

#include <vector>
#include <string>

namespace {

using namespace madrona;
using namespace madrona::phys;
using contactprobe::SimObject;

// Cube: the unit-cube hull; Plane; Sphere of radius 0.7
ObjectManager *loadObjects(const SimCreateArgs &args)
{
    simmgr::RigidBodySet set((size_t)SimObject::NumObjects);
    const uint32_t cube = set.addHull(simmgr::HullSource::box(-0.5f, 0.5f));
    set.hull(SimObject::Cube, cube, 1.f, { 0.5f, 0.5f });
    set.plane(SimObject::Plane);
    set.sphere(SimObject::Sphere, 0.7f, 1.f, { 0.5f, 0.5f });
    return set.load(args, 4);
}

}

struct SimTraits {
    using Sim = contactprobe::Sim;
    using Engine = contactprobe::Engine;

    static constexpr uint32_t numExports = (uint32_t)contactprobe::ExportID::NumExports;
    // (the probes exist on the HIP backend only: sim.cpp)
#ifdef SIM_BACKEND_REF_CPU
    static constexpr uint32_t numTaskGraphs = 1;
#else
    static constexpr uint32_t numTaskGraphs =
        (uint32_t)contactprobe::TaskGraphID::NumTaskGraphs;
#endif
    // sim_step replays task graph 0 only (the others are test probes)
    static constexpr bool stepIsTaskGraph0 = true;

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
                    (uint32_t)contactprobe::ExportID::StepCount });
}

// what the definition of a contact reads (madrona_amd/contact_ref.py)
template <typename T>
void SimTraits::describeColumns(T &cols)
{
    using namespace contactprobe;
    using madrona::Entity;
    using namespace madrona::phys;
    using madrona::base::Scale;
    using madrona::base::ObjectID;

    cols.template add<Body, Entity>("Body.Entity", false);
    cols.template add<Body, Position>("Body.Position", true);
    cols.template add<Body, Rotation>("Body.Rotation", true);
    cols.template add<Body, Scale>("Body.Scale", true);
    cols.template add<Body, ObjectID>("Body.ObjectID", false);
    cols.template add<Body, ResponseType>("Body.ResponseType", false);
    cols.template add<Body, Velocity>("Body.Velocity", true);
#ifndef SIM_BACKEND_REF_CPU
    // the poses the solver's last substep built its contacts at: the reference
    // keeps the component out of its public headers
    cols.template add<Body, xpbd::PreSolvePositional>("Body.PreSolvePositional", true);
#endif
}
