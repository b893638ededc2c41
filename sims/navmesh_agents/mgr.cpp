#include "navmesh_agents/sim.hpp"
#include "navmesh_agents/meshes.hpp"

struct SimTraits;
#include "common/sim_c_api.h"

#include <vector>
#include <string>

namespace simmgr { struct TensorDesc; struct ColumnList; }

struct SimTraits {
    using Sim = navmesh_agents::Sim;
    using Engine = navmesh_agents::Engine;

    static constexpr uint32_t numExports =
        (uint32_t)navmesh_agents::ExportID::NumExports;
    static constexpr uint32_t numTaskGraphs = 1;

    static Sim::Config makeConfig(const SimCreateArgs &args)
    {
        return Sim::Config { args.seed, args.world_base, args.flags };
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
    using navmesh_agents::ExportID;
    int64_t W = num_worlds;
    int64_t A = navmesh_agents::kAgentsPerWorld;
    // mixed float / integer fields: exported as raw 32-bit words
    out.push_back({ "position", SIM_I32, { W, A, 4 }, (uint32_t)ExportID::Position });
    out.push_back({ "goal", SIM_I32, { W, A, 4 }, (uint32_t)ExportID::Goal });
    out.push_back({ "dijkstra", SIM_I32, { W, A, 3 }, (uint32_t)ExportID::Dijkstra });
    out.push_back({ "bfs", SIM_I32, { W, A, 2 }, (uint32_t)ExportID::Bfs });
}

template <typename T>
void SimTraits::describeColumns(T &cols)
{
    using namespace navmesh_agents;
    cols.template add<Agent, madrona::Entity>("Agent.Entity", false);
    cols.template add<Agent, NavPosition>("Agent.NavPosition", false);
    cols.template add<Agent, NavGoal>("Agent.NavGoal", false);
    cols.template add<Agent, DijkstraStats>("Agent.DijkstraStats", false);
    cols.template add<Agent, BfsStats>("Agent.BfsStats", false);
    cols.template add<Agent, AgentInfo>("Agent.AgentInfo", false);
}

// The polygons world `global_world` builds its navmesh from (meshes.hpp), for
// the tests' restatement.  Buffers hold navmesh_agents::kMaxVerts vertices
// (xyz), kMaxPolyIdxs indices and kMaxPolys offsets / sizes; counts receives
// { vertices, indices, polygons }.  Returns the mesh family.
extern "C" SIM_API int32_t sim_navmesh_polygons(uint32_t global_world,
                                                uint32_t seed, uint32_t flags,
                                                float *vertices, uint32_t *idxs,
                                                uint32_t *offsets,
                                                uint32_t *sizes,
                                                uint32_t *counts)
{
    using namespace navmesh_agents;
    std::vector<madrona::math::Vector3> verts(kMaxVerts);
    std::vector<uint32_t> work(kWorkWords);
    PolygonSet polys {};
    polys.verts = verts.data();
    polys.idxs = idxs;
    polys.offsets = offsets;
    polys.sizes = sizes;
    polys.work = work.data();

    uint32_t family = meshFamily(global_world, seed, flags);
    generatePolygons(family,
                     meshKeyOf(worldKeyOf(seed, global_world)), polys);
    for (uint32_t i = 0; i < polys.numVerts; i++) {
        vertices[3 * i] = verts[i].x;
        vertices[3 * i + 1] = verts[i].y;
        vertices[3 * i + 2] = verts[i].z;
    }
    counts[0] = polys.numVerts;
    counts[1] = polys.numIdxs;
    counts[2] = polys.numPolys;
    return (int32_t)family;
}
