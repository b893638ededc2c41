// Standalone broadphase: bodies move kinematically, the BVH is kept up to date
// and the overlapping pairs are left in the CandidateTemporary table for the
// test to read (PhysicsSystem::setupStandaloneBroadphaseOverlapTasks /
// ...CleanupTasks -- the API gpu_hideseek-style simulators use without the
// solver).  Two rigid-body archetypes so that candidate order across
// archetypes is exercised; periodic BVH resets exercise the rebuild.
//
// flags bit 0 ("ray mode"): the number of boxes differs per world (10 .. 100: trees
// of more than 64 leaves next to small ones) and every world holds 1 .. 3
// sensors that each cast a fan of 32 rays through the world's BVH
// (BVH::traceRay; on the MI355X backend the rays of a fan share their origin:
// BVH::traceRayShared, 32 lanes per sensor, so that the two halves of a
// wavefront regularly work on different trees with different leaf counts).
//
// flags bit 1 ("plan mode", DESIGN.md "Broadphase plan mode"): the leaf count of
// a world comes from plan::leafTable (cycled over the GLOBAL world index: a
// small tree next to a large one in every pair of adjacent worlds), the bodies
// sit in one of the layouts below (coordinates from small integers and binary
// fractions: centres tie on purpose), the BVH is sized by a flag field and
// rebuilt every 4 steps, and next to the ray fan every sensor casts 8 of its rays
// through plain BVH::traceRay (RayFanPlain) and every world asks four box
// queries, once with 32 and once with 64 lanes per world (Probe32 / Probe64).
//   bit 2        no world has pillars (the Pillar table stays empty)
//   bits 4-5     max_leaves handed to PhysicsSystem::init: 0 exact (max(L, 1)),
//                1: 64 for L <= 64, 2: 65 for L <= 64 (larger worlds: exact)
//   bits 8-10    layout (plan::Layout)
#pragma once

#include <madrona/taskgraph_builder.hpp>
#include <madrona/custom_context.hpp>
#include <madrona/components.hpp>
#include <madrona/math.hpp>
#include <madrona/rand.hpp>
#include <madrona/physics.hpp>

namespace bponly {

using madrona::Entity;
using madrona::base::Position;
using madrona::math::Vector3;

namespace consts {
inline constexpr int32_t numBoxes = 14;          // (flags bit 0 clear)
inline constexpr int32_t rayModeMaxBoxes = 100;  // (flags bit 0: 10 .. 100 boxes)
inline constexpr int32_t maxBoxes = 130;
inline constexpr int32_t maxSensors = 3;
inline constexpr int32_t raysPerSensor = 32;
inline constexpr int32_t numPillars = 4;
inline constexpr float arena = 5.f;
inline constexpr float deltaT = 0.05f;
inline constexpr int32_t rebuildPeriod = 16;
inline constexpr int32_t planRebuildPeriod = 4;
inline constexpr int32_t plainRays = 8;
inline constexpr int32_t numProbeBoxes = 4;
}

namespace plan {
inline constexpr uint32_t flagRays = 1u << 0;
inline constexpr uint32_t flagPlan = 1u << 1;
inline constexpr uint32_t flagNoPillars = 1u << 2;
inline constexpr uint32_t maxLeavesShift = 4;     // 2 bits
inline constexpr uint32_t layoutShift = 8;        // 3 bits
// MI355X backend only (tests of BroadphaseInputs::CarriedOver, physics.hpp):
// a CarriedOver broadphase opens the step, in front of the drift -- nothing
// between the step's own broadphase and it writes a body ...
inline constexpr uint32_t flagCarried = 1u << 12;
// ... unless this is set: a node in front of it moves each world's first box
// (a broken promise, for MADRONA_MWHIP_CARRY_BROADPHASE=2 to find)
inline constexpr uint32_t flagCarriedNudge = 1u << 13;
// the boxes' Position column is exported: every replay stays full
inline constexpr uint32_t flagExportPosition = 1u << 15;

enum class MaxLeaves : uint32_t { Exact = 0, Staged64 = 1, InPlace65 = 2 };

enum class Layout : uint32_t {
    Drift = 0,        // random drifting boxes (as in ray mode)
    Coincident = 1,   // all boxes identical in position and size
    Line = 2,         // equal spacing along x, equal sizes
    Lattice = 3,      // k x k grid, equal x and y extents: the axis choice
                      // falls through to z, where all centres are equal
    Outlier = 4,      // all boxes coincident but one far away
    Nested = 5,       // one centre, growing sizes
    Doubling = 6,     // centres at 1, 2, 4, 8, ... (/ 64) along x; only worlds of
                      // L <= doublingMaxLeaves, always with max_leaves = 64
                      // (larger worlds: Line) -- the skew overruns the
                      // reference's node array at max_leaves = L
    NumLayouts,
};

inline constexpr int32_t doublingMaxLeaves = 12;

// leaves (boxes + pillars) per world, cycled over the global world index
// (tables live in functions: the world constructor runs on the device too)
inline constexpr int32_t leafTableSize = 28;
inline int32_t leafCount(uint32_t global_world)
{
    const int32_t table[leafTableSize] = {
        0, 130, 1, 97, 2, 66, 3, 65, 4, 64, 5, 63, 6, 62, 8, 61, 9, 60, 16, 33,
        17, 32, 20, 31, 21, 129, 96, 128,
    };
    return table[global_world % (uint32_t)leafTableSize];
}
// 4 pillars where L >= pillarMinLeaves (and flagNoPillars is clear)
inline constexpr int32_t pillarMinLeaves = 8;

// the fan's rays that are cast through plain BVH::traceRay as well
inline int32_t plainRayIndex(int32_t k)
{
    const int32_t table[consts::plainRays] = { 0, 1, 2, 3, 4, 9, 18, 27 };
    return table[k];
}
// half extents of the four query boxes; the last contains everything
inline float probeHalf(int32_t k)
{
    const float table[consts::numProbeBoxes] = { 0.4f, 1.f, 3.f, 50.f };
    return table[k];
}
}

enum class ExportID : uint32_t { StepCount, BoxPosition, NumExports };

struct Drift { Vector3 v; };
struct StepCount { int32_t n; };

// what a sensor's rays met: distance (0: nothing within reach), the entity id
// and the surface normal
struct RayFan {
    float hitT[consts::raysPerSensor];
    int32_t hitEntity[consts::raysPerSensor];
    Vector3 hitNormal[consts::raysPerSensor];
};

// (plan mode) plan::plainRayIndices of the fan through plain BVH::traceRay
struct RayFanPlain {
    float hitT[consts::plainRays];
    int32_t hitEntity[consts::plainRays];
    Vector3 hitNormal[consts::plainRays];
};

// (plan mode) per world: the id of the first dynamic entity
// findEntitiesWithinAABB reports in each of the four query boxes (-1: none);
// on the MI355X backend asked by 32 / by 64 lanes per world
struct Probe32 { int32_t found[consts::numProbeBoxes]; };
struct Probe64 { int32_t found[consts::numProbeBoxes]; };

struct Box : public madrona::Archetype<madrona::phys::RigidBody, Drift> {};
struct Pillar : public madrona::Archetype<madrona::phys::RigidBody> {};
struct Sensor : public madrona::Archetype<Position, Drift, RayFan, RayFanPlain> {};
struct Prober : public madrona::Archetype<Probe32, Probe64> {};

class Engine;

struct Sim : public madrona::WorldBase {
    struct Config {
        uint32_t seed;
        uint32_t worldBase;
        madrona::phys::ObjectManager *rigidBodyObjMgr;
        uint32_t flags;
    };
    struct WorldInit {};

    static void registerTypes(madrona::ECSRegistry &registry, const Config &cfg);
    static void setupTasks(madrona::TaskGraphManager &taskgraph_mgr,
                           const Config &cfg);

    Sim(Engine &ctx, const Config &cfg, const WorldInit &init);

    void initPlanWorld(Engine &ctx, const Config &cfg, uint32_t global_world,
                       madrona::RNG &rng);
    void makeDriftingBox(Engine &ctx, madrona::RNG &rng, int32_t i);
    Entity makeSensor(Engine &ctx, madrona::RNG &rng);

    Entity boxes[consts::maxBoxes];
    Entity pillars[consts::numPillars];
    int32_t numBoxes;
    int32_t numPillars;
    int32_t rebuildPeriod;
    // (plan mode)
    uint32_t flags;
    Entity sensors[consts::maxSensors];
    int32_t numSensors;
};

class Engine : public madrona::CustomContext<Engine, Sim> {
public:
    using CustomContext::CustomContext;
};

}
