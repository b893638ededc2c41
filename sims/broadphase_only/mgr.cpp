#include "broadphase_only/sim.hpp"

#include "common/rigid_body_set.hpp"

#ifdef SIM_BACKEND_REF_CPU
// the candidate archetype is private to the reference's physics sources
#include <physics_impl.hpp>
#endif

#include <vector>
#include <string>

namespace {

using namespace madrona;
using namespace madrona::phys;

ObjectManager *loadCube(const SimCreateArgs &args)
{
    simmgr::RigidBodySet set(1);
    const uint32_t cube = set.addHull(simmgr::HullSource::box(-0.5f, 0.5f));
    set.hull(0, cube, 1.f, { 0.5f, 0.5f });
    return set.load(args, 4);
}

}

struct SimTraits {
    using Sim = bponly::Sim;
    using Engine = bponly::Engine;

    static constexpr uint32_t numExports = (uint32_t)bponly::ExportID::NumExports;
    static constexpr uint32_t numTaskGraphs = 1;

    static Sim::Config makeConfig(const SimCreateArgs &args)
    {
        return Sim::Config { args.seed, args.world_base, loadCube(args), args.flags };
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
                    (uint32_t)bponly::ExportID::StepCount });
}

template <typename T>
void SimTraits::describeColumns(T &cols)
{
    using namespace bponly;
    using madrona::Entity;
    using madrona::phys::CandidateTemporary;
    using madrona::phys::CandidateCollision;

    cols.template add<Box, Entity>("Box.Entity", false);
    cols.template add<Box, Position>("Box.Position", true);
    cols.template add<Box, madrona::phys::broadphase::LeafID>("Box.LeafID", false);
    cols.template add<Pillar, Entity>("Pillar.Entity", false);
    cols.template add<Sensor, Position>("Sensor.Position", true);
    cols.template add<Sensor, RayFan>("Sensor.RayFan", false);
    cols.template add<CandidateTemporary, CandidateCollision>(
        "Candidates.CandidateCollision", false);
    // (plan mode's outputs and what its tests rebuild the leaf boxes from;
    // behind the columns above, whose indices stay)
    cols.template add<Sensor, RayFanPlain>("Sensor.RayFanPlain", false);
    cols.template add<Prober, Probe32>("Prober.Probe32", false);
    cols.template add<Prober, Probe64>("Prober.Probe64", false);
    cols.template add<Box, madrona::phys::Velocity>("Box.Velocity", true);
    cols.template add<Box, madrona::base::Scale>("Box.Scale", true);
    cols.template add<Pillar, madrona::phys::broadphase::LeafID>(
        "Pillar.LeafID", false);
}
