#include "sim.hpp"

#ifdef MADRONA_GPU_MODE
#include <madrona/mw_gpu_entry.hpp>
#endif

using namespace madrona;
using namespace madrona::math;

namespace mesh_cast {

// cos / sin of k * 24 degrees, k = 0 .. 14, as literals: the fan must not
// depend on a math library
static constexpr float kFanCos[kNumRays - 1] = {
    1.f, 0.91354546f, 0.66913061f, 0.30901699f, -0.10452846f, -0.5f,
    -0.80901699f, -0.9781476f, -0.9781476f, -0.80901699f, -0.5f,
    -0.10452846f, 0.30901699f, 0.66913061f, 0.91354546f,
};
static constexpr float kFanSin[kNumRays - 1] = {
    0.f, 0.40673664f, 0.74314483f, 0.95105652f, 0.9945219f, 0.8660254f,
    0.58778525f, 0.20791169f, -0.20791169f, -0.58778525f, -0.8660254f,
    -0.9945219f, -0.95105652f, -0.74314483f, -0.40673664f,
};

static inline RandKey worldKeyOf(uint32_t seed, uint32_t global_world)
{
    return rand::split_i(rand::initKey(seed), global_world);
}

// key of agent `agent`'s draws in step `step`
static inline RandKey agentKeyOf(RandKey world_key, uint32_t step,
                                 uint32_t agent)
{
    return rand::split_i(rand::split_i(world_key, step), agent);
}

static inline float uniformIn(RandKey k, uint32_t i, float lo, float hi)
{
    return lo + (hi - lo) * rand::sampleUniform(rand::split_i(k, i));
}

static inline void placeAgent(RandKey k, AgentPos &pos)
{
    pos.x = uniformIn(k, 10, -3.5f, 3.5f);
    pos.y = uniformIn(k, 11, -3.5f, 3.5f);
    pos.z = uniformIn(k, 12, 0.3f, 2.5f);
}

void Sim::registerTypes(ECSRegistry &registry, const Config &)
{
    registry.registerComponent<AgentPos>();
    registry.registerComponent<RayT>();
    registry.registerComponent<RayMaterial>();
    registry.registerComponent<RayNormal>();
    registry.registerComponent<RayUV>();
    registry.registerComponent<SweepResult>();
    registry.registerComponent<OverlapResult>();
    registry.registerComponent<AgentInfo>();

    registry.registerArchetype<Agent>();

    registry.exportColumn<Agent, AgentPos>((uint32_t)ExportID::Position);
    registry.exportColumn<Agent, SweepResult>((uint32_t)ExportID::Sweep);
    registry.exportColumn<Agent, OverlapResult>((uint32_t)ExportID::Overlap);
    registry.exportColumn<Agent, RayT>((uint32_t)ExportID::RayT);
}

inline void castRays(Engine &ctx,
                     AgentPos &pos,
                     AgentInfo &info,
                     RayT &ray_t,
                     RayMaterial &ray_mat,
                     RayNormal &ray_n,
                     RayUV &ray_uv)
{
    const MeshBVH &mesh = *ctx.data().mesh;
    RandKey k = agentKeyOf(ctx.data().worldKey, info.step, info.idx);

    float hx = uniformIn(k, 0, -1.f, 1.f);
    float hy = uniformIn(k, 1, -1.f, 1.f);
    if (hx == 0.f && hy == 0.f) {
        hx = 1.f;
    }

    int32_t stack[kRayStackSize];

    for (uint32_t r = 0; r < kNumRays; r++) {
        Vector3 o, d;
        float t_max = FLT_MAX;
        if (r + 1 < kNumRays) {
            o = Vector3 { pos.x, pos.y, pos.z };
            d = Vector3 {
                hx * kFanCos[r] - hy * kFanSin[r],
                hx * kFanSin[r] + hy * kFanCos[r],
                0.2f - 0.1f * (float)r,
            };
            if (r == kShortRay) {
                t_max = kShortRayTMax;
            }
        } else {
            // straight down onto the nearest integer grid point
            o = Vector3 { floorf(pos.x + 0.5f), floorf(pos.y + 0.5f),
                          kProbeHeight };
            d = Vector3 { 0.f, 0.f, -1.f };
        }

        MeshBVH::HitInfo hit;
        int32_t stack_size = 0;
        bool did_hit = mesh.traceRay(o, d, &hit, stack, stack_size, t_max);

        if (did_hit) {
            ray_t.tBits[r] = __builtin_bit_cast(uint32_t, hit.tHit);
            ray_mat.mat[r] = mesh.getMaterialIDX(hit);
            ray_n.n[r][0] = hit.normal.x;
            ray_n.n[r][1] = hit.normal.y;
            ray_n.n[r][2] = hit.normal.z;
            ray_uv.uv[r][0] = hit.uv.x;
            ray_uv.uv[r][1] = hit.uv.y;
        } else {
            ray_t.tBits[r] = 0xFFFF'FFFFu;
            ray_mat.mat[r] = 0xFFFF'FFFFu;
            ray_n.n[r][0] = 0.f;
            ray_n.n[r][1] = 0.f;
            ray_n.n[r][2] = 0.f;
            ray_uv.uv[r][0] = 0.f;
            ray_uv.uv[r][1] = 0.f;
        }
    }
}

inline void sweepAgent(Engine &ctx,
                       AgentPos &pos,
                       AgentInfo &info,
                       SweepResult &sweep)
{
    MeshBVH &mesh = *ctx.data().mesh;
    RandKey k = agentKeyOf(ctx.data().worldKey, info.step, info.idx);

    Vector3 move {
        uniformIn(k, 2, -1.5f, 1.5f),
        uniformIn(k, 3, -1.5f, 1.5f),
        uniformIn(k, 4, -0.9f, 0.3f),
    };

    Vector3 normal { 0.f, 0.f, 0.f };
    float t = mesh.sphereCast(Vector3 { pos.x, pos.y, pos.z }, move,
                              pos.radius, &normal, 1.f);

    sweep = SweepResult { t, normal.x, normal.y, normal.z };

    pos.x += move.x * t;
    pos.y += move.y * t;
    pos.z += move.z * t;
}

inline void overlapAgent(Engine &ctx,
                         AgentPos &pos,
                         OverlapResult &overlap)
{
    const MeshBVH &mesh = *ctx.data().mesh;

    const float h = kOverlapHalfExtent;
    AABB box {
        Vector3 { pos.x - h, pos.y - h, pos.z - h },
        Vector3 { pos.x + h, pos.y + h, pos.z + h },
    };

    uint32_t num_tris = 0;
    Vector3 sum { 0.f, 0.f, 0.f };
    mesh.findOverlaps(box, [&](Vector3 va, Vector3 vb, Vector3 vc) {
        num_tris++;
        sum = sum + va;
        sum = sum + vb;
        sum = sum + vc;
    });

    overlap = OverlapResult { num_tris, sum.x, sum.y, sum.z };
}

// after the queries: the step counter, and a new place every few steps
inline void advanceAgent(Engine &ctx,
                         AgentPos &pos,
                         AgentInfo &info)
{
    info.step += 1;
    if (info.step % kResampleEvery == 0) {
        placeAgent(agentKeyOf(ctx.data().worldKey, info.step, info.idx), pos);
    }
}

void Sim::setupTasks(TaskGraphManager &taskgraph_mgr, const Config &)
{
    TaskGraphBuilder &builder = taskgraph_mgr.init(0);

    auto rays = builder.addToGraph<ParallelForNode<Engine, castRays,
        AgentPos, AgentInfo, RayT, RayMaterial, RayNormal, RayUV>>({});
    auto sweep = builder.addToGraph<ParallelForNode<Engine, sweepAgent,
        AgentPos, AgentInfo, SweepResult>>({rays});
    auto overlap = builder.addToGraph<ParallelForNode<Engine, overlapAgent,
        AgentPos, OverlapResult>>({sweep});
    builder.addToGraph<ParallelForNode<Engine, advanceAgent,
        AgentPos, AgentInfo>>({overlap});
}

Sim::Sim(Engine &ctx, const Config &cfg, const WorldInit &)
    : WorldBase(ctx)
{
    uint32_t global_world = cfg.worldBase + (uint32_t)ctx.worldID().idx;
    worldKey = worldKeyOf(cfg.seed, global_world);
    mesh = cfg.meshes + global_world % cfg.numMeshes;

    for (uint32_t i = 0; i < kAgentsPerWorld; i++) {
        Entity agent = ctx.makeEntity<Agent>();
        AgentPos &pos = ctx.get<AgentPos>(agent);
        // a thin and a fat sphere
        pos.radius = i % 2 == 0 ? 0.05f : 0.5f;
        placeAgent(agentKeyOf(worldKey, 0xFFFF'0000u, i), pos);

        ctx.get<AgentInfo>(agent) = AgentInfo { i, 0 };
        ctx.get<RayT>(agent) = RayT {};
        ctx.get<RayMaterial>(agent) = RayMaterial {};
        ctx.get<RayNormal>(agent) = RayNormal {};
        ctx.get<RayUV>(agent) = RayUV {};
        ctx.get<SweepResult>(agent) = SweepResult { 0.f, 0.f, 0.f, 0.f };
        ctx.get<OverlapResult>(agent) = OverlapResult { 0, 0.f, 0.f, 0.f };
    }
}

#ifdef MADRONA_GPU_MODE
MADRONA_BUILD_MWGPU_ENTRY(Engine, Sim, Sim::Config, Sim::WorldInit);
#endif

}
