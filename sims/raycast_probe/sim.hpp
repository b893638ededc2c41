// Ray-caster probe simulator: static worlds, one scene kind per world
// (world w builds kind w % 16), each an edge of the batch ray caster
// (madrona_amd/csrc/render_raycast.hip) that no other simulator's scenes reach:
// instance counts 0, 1, 2 and either side of 64, equal Morton codes, a deep
// top-level tree, a camera inside an instance, instances behind the cameras,
// 0 / 8 / 9 lights, spot cones, and a frustum every tile of which sees another
// subset.  Two viewers per world: one axis-aligned with a 90 degree field of
// view, one generally rotated with 60 degrees and a camera offset.  Stepped
// through madrona::render::RenderingSystem like sims/render_prep; compiled
// unchanged against the reference CPU backend (records go to RenderECSBridge
// buffers) and against the HIP backend.  tests/test_raycast_probe_{cpu,gpu}.py.
#pragma once

#include <madrona/taskgraph_builder.hpp>
#include <madrona/custom_context.hpp>
#include <madrona/components.hpp>
#include <madrona/render/ecs.hpp>

namespace raycastprobe {

using madrona::Entity;
using madrona::base::ObjectID;
using madrona::base::Position;
using madrona::base::Rotation;
using madrona::base::Scale;

namespace consts {
inline constexpr int32_t numKinds = 16;
inline constexpr int32_t numViewers = 2;
// box, ellipsoid (168 triangles), cylinder, wedge (per-triangle materials,
// textured), sheared box (12 triangles, not its own bounding box)
inline constexpr int32_t numObjects = 5;
// the deep-tree kind: pairs of codes (1 << (29 - k)) | {0, 1}, k = 0 .. pairs - 1
inline constexpr int32_t deepPairs = 17;
inline constexpr int32_t tooDeepPairs = 27;
// and this many more with codes (3 << 28) | j, j = 2 ..: next to the root
inline constexpr int32_t deepFillers = 32;
inline constexpr int32_t maxInstances = 96;
}

enum class ExportID : uint32_t {
    Steps,
    // ray caster outputs, one row per view (HIP backend)
    RGB,
    Depth,
    NumExports,
};

struct StepCount {
    int32_t steps;
};

struct Thing : public madrona::Archetype<
    Position, Rotation, Scale, ObjectID,
    madrona::render::Renderable,
    madrona::render::MaterialOverride,
    madrona::render::ColorOverride
> {};

struct Viewer : public madrona::Archetype<
    Position, Rotation,
    madrona::render::RenderCamera
> {};

struct Lamp : public madrona::Archetype<
    Position,
    madrona::render::LightDescDirection,
    madrona::render::LightDescType,
    madrona::render::LightDescShadow,
    madrona::render::LightDescCutoffAngle,
    madrona::render::LightDescIntensity,
    madrona::render::LightDescActive,
    madrona::render::LightCarrier
> {};

class Engine;

struct Sim : public madrona::WorldBase {
    struct Config {
        uint32_t worldBase;
        // kind 8 with consts::tooDeepPairs levels: deeper than the ray
        // caster's traversal stack
        uint32_t tooDeep;
        // reference CPU backend: the buffers its systems append to
        const madrona::render::RenderECSBridge *bridge;
    };

    struct WorldInit {};

    static void registerTypes(madrona::ECSRegistry &registry,
                              const Config &cfg);
    static void setupTasks(madrona::TaskGraphManager &taskgraph_mgr,
                           const Config &cfg);

    Sim(Engine &ctx, const Config &cfg, const WorldInit &init);

    int32_t kind;
};

class Engine : public madrona::CustomContext<Engine, Sim> {
public:
    using CustomContext::CustomContext;
};

}
