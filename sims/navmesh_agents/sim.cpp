#include "sim.hpp"
#include "meshes.hpp"

#ifdef MADRONA_GPU_MODE
#include <madrona/mw_gpu_entry.hpp>
#endif

using namespace madrona;
using namespace madrona::math;

namespace navmesh_agents {

// FNV-1a over whole 32-bit words
inline constexpr uint32_t kHashBasis = 2166136261u;
inline constexpr uint32_t kHashPrime = 16777619u;

static inline void sampleAgent(Sim &sim, const AgentInfo &info,
                               NavPosition &pos, NavGoal &goal)
{
    // (an empty mesh: a constructor pass whose memory did not fit, which the
    // executor runs again)
    if (sim.navmesh.numTris == 0) {
        pos = NavPosition { 0.f, 0.f, 0.f, 0 };
        goal = NavGoal { 0.f, 0.f, 0.f, 0 };
        return;
    }

    RandKey k = agentKeyOf(sim.worldKey, info.epoch, info.idx);

    uint32_t poly;
    Vector3 p = sim.navmesh.samplePointAndPoly(rand::split_i(k, 0), &poly);
    pos = NavPosition { p.x, p.y, p.z, poly };

    Vector3 g = sim.navmesh.samplePointAndPoly(rand::split_i(k, 1), &poly);
    goal = NavGoal { g.x, g.y, g.z, poly };
}

void Sim::registerTypes(ECSRegistry &registry, const Config &)
{
    registry.registerComponent<NavPosition>();
    registry.registerComponent<NavGoal>();
    registry.registerComponent<DijkstraStats>();
    registry.registerComponent<BfsStats>();
    registry.registerComponent<AgentInfo>();

    registry.registerArchetype<Agent>();

    registry.exportColumn<Agent, NavPosition>((uint32_t)ExportID::Position);
    registry.exportColumn<Agent, NavGoal>((uint32_t)ExportID::Goal);
    registry.exportColumn<Agent, DijkstraStats>((uint32_t)ExportID::Dijkstra);
    registry.exportColumn<Agent, BfsStats>((uint32_t)ExportID::Bfs);
}

// every kResampleEvery steps a new spawn point and goal
inline void resampleAgents(Engine &ctx,
                           NavPosition &pos,
                           NavGoal &goal,
                           AgentInfo &info)
{
    info.step += 1;
    if (info.step % kResampleEvery == 0) {
        info.epoch += 1;
        sampleAgent(ctx.data(), info, pos, goal);
    }
}

// Dijkstra from the agent's polygon and position over the whole mesh; the
// search state is scratch memory (freed by the ResetTmpAlloc node after this)
inline void agentDijkstra(Engine &ctx,
                          NavPosition &pos,
                          NavGoal &goal,
                          DijkstraStats &stats)
{
    Navmesh &nav = ctx.data().navmesh;
    const uint64_t num_tris = nav.numTris;
    if (num_tris == 0) {
        stats = DijkstraStats { 0.f, 0, 0 };
        return;
    }

    char *buf = (char *)ctx.tmpAlloc(num_tris *
        (sizeof(Vector3) + sizeof(float) + 2 * sizeof(uint32_t)));
    Navmesh::DijkstrasState state {
        (float *)(buf + num_tris * sizeof(Vector3)),
        (Vector3 *)buf,
        (uint32_t *)(buf + num_tris * (sizeof(Vector3) + sizeof(float))),
        (uint32_t *)(buf + num_tris * (sizeof(Vector3) + 2 * sizeof(float))),
    };

    uint32_t num_popped = 0;
    uint32_t hash = kHashBasis;
    nav.dijkstrasFromPoly(pos.poly, Vector3 { pos.x, pos.y, pos.z }, state,
        [&](uint32_t poly, Vector3, float) {
            num_popped++;
            hash = (hash ^ poly) * kHashPrime;
        });

    stats = DijkstraStats { state.distances[goal.poly], num_popped, hash };
}

// BFS from the agent's polygon that expands polygons whose centroid lies
// within the radius around the agent
inline void agentBfs(Engine &ctx,
                     NavPosition &pos,
                     BfsStats &stats)
{
    Navmesh &nav = ctx.data().navmesh;
    const uint64_t num_tris = nav.numTris;
    if (num_tris == 0) {
        stats = BfsStats { 0, 0 };
        return;
    }

    char *buf = (char *)ctx.tmpAlloc(num_tris * (sizeof(uint32_t) + 1));
    Navmesh::BFSState state {
        (uint32_t *)buf,
        (bool *)(buf + num_tris * sizeof(uint32_t)),
    };

    const Vector3 center { pos.x, pos.y, pos.z };
    uint32_t num_visited = 0;
    uint32_t hash = kHashBasis;
    nav.bfsFromPoly(pos.poly, state, [&](uint32_t poly) {
        num_visited++;
        hash = (hash ^ poly) * kHashPrime;

        Vector3 a, b, c;
        nav.getTriangleVertices(poly, &a, &b, &c);
        Vector3 centroid = (a + b + c) * (1.f / 3.f);
        return (centroid - center).length2() <= kBfsRadius2;
    });

    stats = BfsStats { num_visited, hash };
}

void Sim::setupTasks(TaskGraphManager &taskgraph_mgr, const Config &)
{
    TaskGraphBuilder &builder = taskgraph_mgr.init(0);

    auto resample = builder.addToGraph<ParallelForNode<Engine, resampleAgents,
        NavPosition, NavGoal, AgentInfo>>({});
    auto dijkstra = builder.addToGraph<ParallelForNode<Engine, agentDijkstra,
        NavPosition, NavGoal, DijkstraStats>>({resample});
    auto reset_tmp = builder.addToGraph<ResetTmpAllocNode>({dijkstra});
    auto bfs = builder.addToGraph<ParallelForNode<Engine, agentBfs,
        NavPosition, BfsStats>>({reset_tmp});
    builder.addToGraph<ResetTmpAllocNode>({bfs});
}

Sim::Sim(Engine &ctx, const Config &cfg, const WorldInit &)
    : WorldBase(ctx)
{
    uint32_t global_world = cfg.worldBase + (uint32_t)ctx.worldID().idx;
    worldKey = worldKeyOf(cfg.seed, global_world);

    // the polygons only live while the navmesh is built: scratch memory
    char *buf = (char *)ctx.tmpAlloc(sizeof(Vector3) * kMaxVerts +
        sizeof(uint32_t) * (kMaxPolyIdxs + 2 * kMaxPolys + kWorkWords));
    if (mwGPU::allocOverflowed()) {
        // the buffer may be the scratch region's base, which other lanes use:
        // write nothing.  The executor grows the region and runs the
        // constructors again.
        navmesh = Navmesh {};
    } else {
        PolygonSet polys {};
        polys.verts = (Vector3 *)buf;
        polys.idxs = (uint32_t *)(buf + sizeof(Vector3) * kMaxVerts);
        polys.offsets = polys.idxs + kMaxPolyIdxs;
        polys.sizes = polys.offsets + kMaxPolys;
        polys.work = polys.sizes + kMaxPolys;
        generatePolygons(meshFamily(global_world, cfg.seed, cfg.flags),
                         meshKeyOf(worldKey), polys);

        navmesh = Navmesh::initFromPolygons(polys.verts, polys.idxs,
            polys.offsets, polys.sizes, polys.numVerts, polys.numPolys);
    }

    for (uint32_t i = 0; i < kAgentsPerWorld; i++) {
        Entity agent = ctx.makeEntity<Agent>();
        AgentInfo &info = ctx.get<AgentInfo>(agent);
        info = AgentInfo { i, 0, 0 };
        sampleAgent(*this, info, ctx.get<NavPosition>(agent),
                    ctx.get<NavGoal>(agent));
        ctx.get<DijkstraStats>(agent) = DijkstraStats { 0.f, 0, 0 };
        ctx.get<BfsStats>(agent) = BfsStats { 0, 0 };
    }
}

#ifdef MADRONA_GPU_MODE
MADRONA_BUILD_MWGPU_ENTRY(Engine, Sim, Sim::Config, Sim::WorldInit);
#endif

}
