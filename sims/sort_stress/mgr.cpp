#include "sort_stress/sim.hpp"

struct SimTraits;
#include "common/sim_c_api.h"

#include <vector>
#include <string>

struct SimTraits {
    using Sim = sortstress::Sim;
    using Engine = sortstress::Engine;

    static constexpr uint32_t numExports =
        (uint32_t)sortstress::ExportID::NumExports;
    static constexpr uint32_t numTaskGraphs =
        (uint32_t)sortstress::TaskGraphID::NumTaskGraphs;
    // sim_step replays task graph 0 only (the others are test probes)
    static constexpr bool stepIsTaskGraph0 = true;

    static Sim::Config makeConfig(const SimCreateArgs &args)
    {
        return Sim::Config { args.seed, args.world_base, args.flags & 1u,
                             (args.flags >> 1) & 1u,
                             (args.flags >> 2) & 1u,
                             (args.flags >> 3) & 1u,
                             (args.flags >> 4) & 1u,
                             (args.flags >> 5) & 1u,
                             (args.flags >> 6) & 1u,
                             (args.flags >> 7) & 1u,
                             (args.flags >> 8) & 7u };
    }

    static void makeInits(const SimCreateArgs &, Sim::WorldInit *) {}

    template <typename T>
    static void describeTensors(T &out, uint32_t num_worlds);
    template <typename T>
    static void describeFlagTensors(T &out, const SimCreateArgs &args);
    template <typename T>
    static void describeColumns(T &cols);
    template <typename T>
    static void describeFlagColumns(T &cols, const SimCreateArgs &args);
};

#include "common/mgr_impl.inl"

template <typename T>
void SimTraits::describeTensors(T &out, uint32_t num_worlds)
{
    out.push_back({ "churn", SIM_I32, { (int64_t)num_worlds, 3 },
                    (uint32_t)sortstress::ExportID::Churn });
}

// exports that only exist with flags 32 (plan / probe) and 64 (item_vec3),
// HIP backend only
template <typename T>
void SimTraits::describeFlagTensors(T &out, const SimCreateArgs &args)
{
#ifndef SIM_BACKEND_REF_CPU
    using namespace sortstress;
    const int64_t w = (int64_t)args.num_worlds;
    if ((args.flags & 32u) != 0u) {
        out.push_back({ "plan", SIM_I32, { w, 5 }, (uint32_t)ExportID::Plan });
        out.push_back({ "probe", SIM_I32,
                        { w, (int64_t)(sizeof(ProbeOut) / 4) },
                        (uint32_t)ExportID::Probe });
    }
    if ((args.flags & 64u) != 0u) {
        // (the first consts::maxItems rows per world of the column, as many
        // as a table the plan sets up can hold)
        out.push_back({ "item_vec3", SIM_F32, { w * consts::maxItems, 3 },
                        (uint32_t)ExportID::ItemVec3 });
    }
#else
    (void)out; (void)args;
#endif
}

template <typename T>
void SimTraits::describeColumns(T &cols)
{
    using namespace sortstress;
    using madrona::Entity;
    using madrona::WorldID;

    cols.template add<Item, Entity>("Item.Entity", false);
    cols.template add<Item, Tag8>("Item.Tag8", false);
    cols.template add<Item, Half>("Item.Half", false);
    cols.template add<Item, Key>("Item.Key", false);
    cols.template add<Item, Pair>("Item.Pair", false);
    cols.template add<Item, Vec3>("Item.Vec3", true);
    cols.template add<Item, Quad>("Item.Quad", true);
    cols.template add<Item, Blob20>("Item.Blob20", false);
    cols.template add<Item, Wide>("Item.Wide", true);
#ifndef SIM_BACKEND_REF_CPU
    // (the global tables of the HIP backend carry the world id as column 1;
    // the reference CPU backend keeps one table per world)
    cols.template add<Item, WorldID>("Item.WorldID", false);
#endif
    cols.template add<Scratch, Key>("Scratch.Key", false);
    cols.template add<Scratch, Vec3>("Scratch.Vec3", true);
}

// columns of the tables that only exist with flags 128 (Config::reusePlan)
template <typename T>
void SimTraits::describeFlagColumns(T &cols, const SimCreateArgs &args)
{
    using namespace sortstress;
    using madrona::Entity;

    if ((args.flags & 128u) == 0u) {
        return;
    }
    cols.template add<Reuse0, Entity>("Reuse0.Entity", false);
    cols.template add<Reuse0, Key>("Reuse0.Key", false);
    cols.template add<Reuse0, Pair>("Reuse0.Pair", false);
    cols.template add<Reuse1, Entity>("Reuse1.Entity", false);
    cols.template add<Reuse1, Key>("Reuse1.Key", false);
    cols.template add<Reuse1, Pair>("Reuse1.Pair", false);
    cols.template add<Reuse2, Entity>("Reuse2.Entity", false);
    cols.template add<Reuse2, Key>("Reuse2.Key", false);
    cols.template add<Reuse2, Pair>("Reuse2.Pair", false);
    cols.template add<Reuse3, Entity>("Reuse3.Entity", false);
    cols.template add<Reuse3, Key>("Reuse3.Key", false);
    cols.template add<Reuse3, Pair>("Reuse3.Pair", false);
    cols.template add<Reuse4, Entity>("Reuse4.Entity", false);
    cols.template add<Reuse4, Key>("Reuse4.Key", false);
    cols.template add<Reuse4, Pair>("Reuse4.Pair", false);
}
