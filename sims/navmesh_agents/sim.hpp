// Navmesh agents: every world builds a triangle navmesh in its constructor
// (Navmesh::initFromPolygons on the device) from one of the polygon families in
// meshes.hpp; a few agents per world sample spawn points and goals on it, and
// each step run Dijkstra from their polygon (distance to the goal polygon,
// polygons popped, a hash of the pop order) and a BFS bounded by a radius
// around them (polygons visited, a hash of the visit order).  Agents sample
// again every kResampleEvery steps.
//
// The search state is per-step scratch memory (Context::tmpAlloc).  There is
// no reference-CPU build of this simulator: tests/test_navmesh_agents_gpu.py
// runs it in lock step with the numpy restatement (tests/navmesh_restate.py).
#pragma once

#include <madrona/taskgraph_builder.hpp>
#include <madrona/custom_context.hpp>
#include <madrona/navmesh.hpp>
#include <madrona/rand.hpp>

namespace navmesh_agents {

using madrona::Entity;
using madrona::RandKey;

inline constexpr uint32_t kAgentsPerWorld = 4;
inline constexpr uint32_t kResampleEvery = 5;
// BFS accepts (expands) a polygon whose centroid lies within this radius
inline constexpr float kBfsRadius2 = 6.25f;

enum class ExportID : uint32_t {
    Position,
    Goal,
    Dijkstra,
    Bfs,
    NumExports,
};

// agent position and the triangle it stands on
struct NavPosition {
    float x, y, z;
    uint32_t poly;
};

struct NavGoal {
    float x, y, z;
    uint32_t poly;
};

// goalDist: Dijkstra's distance to the goal polygon (FLT_MAX: unreachable);
// popHash: FNV-1a over the pop order
struct DijkstraStats {
    float goalDist;
    uint32_t numPopped;
    uint32_t popHash;
};

struct BfsStats {
    uint32_t numVisited;
    uint32_t visitHash;
};

struct AgentInfo {
    uint32_t idx;       // agent index in its world
    uint32_t epoch;     // how many times it has sampled
    uint32_t step;
};

struct Agent : public madrona::Archetype<
    NavPosition, NavGoal, DijkstraStats, BfsStats, AgentInfo
> {};

class Engine;

struct Sim : public madrona::WorldBase {
    struct Config {
        uint32_t seed;
        uint32_t worldBase;
        uint32_t flags;     // & 7: mesh family (meshes.hpp)
    };

    struct WorldInit {};

    static void registerTypes(madrona::ECSRegistry &registry,
                              const Config &cfg);

    static void setupTasks(madrona::TaskGraphManager &taskgraph_mgr,
                           const Config &cfg);

    Sim(Engine &ctx, const Config &cfg, const WorldInit &init);

    RandKey worldKey;
    madrona::Navmesh navmesh;
};

class Engine : public madrona::CustomContext<Engine, Sim> {
public:
    using CustomContext::CustomContext;
};

// keys: the world's, its mesh's, and an agent's samples in one epoch
inline RandKey worldKeyOf(uint32_t seed, uint32_t global_world)
{
    return madrona::rand::split_i(madrona::rand::initKey(seed), global_world);
}

inline RandKey meshKeyOf(RandKey world_key)
{
    return madrona::rand::split_i(world_key, 0xFFFF'0000u);
}

inline RandKey agentKeyOf(RandKey world_key, uint32_t epoch, uint32_t agent)
{
    return madrona::rand::split_i(madrona::rand::split_i(world_key, epoch),
                                  agent);
}

}
