// A probe for contact queries (mwhip_contacts_*): rigid bodies of
// one archetype under XPBD in worlds shaped to produce every kind of contact
// the narrowphase builds -- hull-hull face contacts with either body as the
// reference, edge contacts, hull-plane manifolds, sphere-hull contacts -- and
// the worlds a query must get right besides: only static bodies, no bodies,
// more than 64 bodies.  Its dump list has what the definition of a contact
// reads, Scale, ObjectID and ResponseType included.  Compiled unchanged against
// the reference CPU backend (oracle) and the HIP backend.  (On the HIP backend
// two more task graphs, test probes, leave the Body table unsorted and sort it
// again: TaskGraphID.)
#pragma once

#include <madrona/taskgraph_builder.hpp>
#include <madrona/custom_context.hpp>
#include <madrona/components.hpp>
#include <madrona/math.hpp>
#include <madrona/rand.hpp>
#include <madrona/physics.hpp>

namespace contactprobe {

using madrona::Entity;
using madrona::base::Position;
using madrona::base::Rotation;
using madrona::math::Vector3;

namespace consts {
inline constexpr float deltaT = 0.04f;
inline constexpr int32_t numSubsteps = 4;
// the world of global index crowdedWorld is the crowded pen; the others go by
// index % 4: a pen, a slab, statics only, nothing
inline constexpr uint32_t crowdedWorld = 5;
inline constexpr int32_t crowdedSide = 6;       // cubes per side of its layers
inline constexpr int32_t crowdedLayers = 2;
}

enum class SimObject : int32_t { Cube, Plane, Sphere, NumObjects };
enum class ExportID : uint32_t { StepCount, NumExports };
// Step is the simulator; the other two are test probes of the HIP backend
// (tests/test_shape_query_gpu.py): AppendOnly gives every world one more static
// cube, far above everything, and sorts nothing, so that the Body table waits
// for its world sort; CompactOnly is the sort it waits for.
enum class TaskGraphID : uint32_t { Step, AppendOnly, CompactOnly, NumTaskGraphs };

struct StepCount { int32_t n; };

struct Body : public madrona::Archetype<madrona::phys::RigidBody> {};

class Engine;

struct Sim : public madrona::WorldBase {
    struct Config {
        uint32_t seed;
        uint32_t worldBase;
        madrona::phys::ObjectManager *rigidBodyObjMgr;
    };
    struct WorldInit {};

    static void registerTypes(madrona::ECSRegistry &registry, const Config &cfg);
    static void setupTasks(madrona::TaskGraphManager &taskgraph_mgr,
                           const Config &cfg);

    Sim(Engine &ctx, const Config &cfg, const WorldInit &init);
};

class Engine : public madrona::CustomContext<Engine, Sim> {
public:
    using CustomContext::CustomContext;
};

}
