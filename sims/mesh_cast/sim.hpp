// Mesh cast: agents that sense and move against static triangle meshes through
// MeshBVH's queries (<madrona/mesh_bvh.hpp>).  The Manager builds the mesh
// families of meshes.hpp once (MeshBVHBuilder), hands them to every world
// through Sim::Config (host pointers on the reference CPU backend, uploaded
// ones on the HIP backend), and world w uses mesh w % numMeshes.
//
// Per step and agent:
//   ray fan   16 traceRay calls: 15 around the agent's heading, tilted further
//             down from one to the next (one of them with a short t_max), and
//             one straight down from z = kProbeHeight above the nearest
//             integer grid point, which over the height field goes exactly
//             through a mesh vertex (the exact-zero barycentric fallback of
//             the triangle test).  Recorded: tHit bits, normal, uv, material.
//   sweep     one sphereCast along the agent's move; the agent advances by the
//             returned t.  Recorded: t and the contact normal.
//   overlap   one findOverlaps over a box around the agent.  Recorded: the
//             triangle count and the fp32 sum of the visited vertices, in
//             visiting order.
// Headings and moves come from the world's RNG key; every kResampleEvery
// steps the agent is put somewhere new.  No trigonometry: everything is +, -,
// *, /, sqrt and the RNG, so the reference CPU backend and the device agree
// bit for bit (tests/test_mesh_bvh_gpu.py).
#pragma once

#include <madrona/taskgraph_builder.hpp>
#include <madrona/custom_context.hpp>
#include <madrona/mesh_bvh.hpp>
#include <madrona/rand.hpp>

namespace mesh_cast {

using madrona::Entity;
using madrona::RandKey;
using madrona::MeshBVH;

inline constexpr uint32_t kAgentsPerWorld = 4;
inline constexpr uint32_t kNumRays = 16;
inline constexpr uint32_t kResampleEvery = 4;
inline constexpr float kProbeHeight = 10.f;
inline constexpr float kOverlapHalfExtent = 0.75f;
// ray kShortRay gives up after this distance
inline constexpr uint32_t kShortRay = 3;
inline constexpr float kShortRayTMax = 1.f;
// traceRay's stack: 32 entries cover any tree of MeshBVHBuilder's
inline constexpr uint32_t kRayStackSize = 32;

enum class ExportID : uint32_t {
    Position,
    Sweep,
    Overlap,
    RayT,
    NumExports,
};

struct AgentPos {
    float x, y, z;
    float radius;
};

// tHit's bits (0xFFFFFFFF: no hit) and the hit's material (0xFFFFFFFF: none)
struct RayT {
    uint32_t tBits[kNumRays];
};

struct RayMaterial {
    uint32_t mat[kNumRays];
};

struct RayNormal {
    float n[kNumRays][3];
};

struct RayUV {
    float uv[kNumRays][2];
};

// t == 1: the move was free, the normal is zero
struct SweepResult {
    float t;
    float nx, ny, nz;
};

struct OverlapResult {
    uint32_t numTris;
    float sumX, sumY, sumZ;
};

struct AgentInfo {
    uint32_t idx;       // agent index in its world
    uint32_t step;
};

struct Agent : public madrona::Archetype<
    AgentPos, RayT, RayMaterial, RayNormal, RayUV, SweepResult, OverlapResult,
    AgentInfo
> {};

class Engine;

struct Sim : public madrona::WorldBase {
    struct Config {
        uint32_t seed;
        uint32_t worldBase;
        MeshBVH *meshes;        // shared by all worlds
        uint32_t numMeshes;
    };

    struct WorldInit {};

    static void registerTypes(madrona::ECSRegistry &registry,
                              const Config &cfg);

    static void setupTasks(madrona::TaskGraphManager &taskgraph_mgr,
                           const Config &cfg);

    Sim(Engine &ctx, const Config &cfg, const WorldInit &init);

    RandKey worldKey;
    MeshBVH *mesh;
};

class Engine : public madrona::CustomContext<Engine, Sim> {
public:
    using CustomContext::CustomContext;
};

}
