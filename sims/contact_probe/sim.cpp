#include "sim.hpp"

#ifdef MADRONA_GPU_MODE
#include <madrona/mw_gpu_entry.hpp>
#endif

using namespace madrona;
using namespace madrona::math;
using namespace madrona::phys;
using madrona::base::Scale;
using madrona::base::ObjectID;

namespace contactprobe {

void Sim::registerTypes(ECSRegistry &registry, const Config &)
{
    base::registerTypes(registry);
    PhysicsSystem::registerTypes(registry);

    registry.registerSingleton<StepCount>();
    registry.registerArchetype<Body>();

    registry.exportSingleton<StepCount>((uint32_t)ExportID::StepCount);
}

static inline Entity makeBody(Engine &ctx, Vector3 pos, Quat rot, Diag3x3 scale,
                              SimObject obj, ResponseType response)
{
    Entity e = ctx.makeEntity<Body>();
    ObjectID obj_id { (int32_t)obj };
    ctx.get<Position>(e) = pos;
    ctx.get<Rotation>(e) = rot;
    ctx.get<Scale>(e) = scale;
    ctx.get<ObjectID>(e) = obj_id;
    ctx.get<ResponseType>(e) = response;
    ctx.get<Velocity>(e) = Velocity { Vector3::zero(), Vector3::zero() };
    ctx.get<ExternalForce>(e) = Vector3::zero();
    ctx.get<ExternalTorque>(e) = Vector3::zero();
    ctx.get<broadphase::LeafID>(e) =
        PhysicsSystem::registerEntity(ctx, e, obj_id);
    return e;
}

inline void countSystem(Engine &, StepCount &steps)
{
    steps.n += 1;
}

#ifdef MADRONA_GPU_MODE
inline void appendSystem(Engine &ctx, StepCount &)
{
    makeBody(ctx, Vector3 { 0.f, 0.f, 200.f }, Quat { 1, 0, 0, 0 },
             Diag3x3 { 1.f, 1.f, 1.f }, SimObject::Cube, ResponseType::Static);
}
#endif

void Sim::setupTasks(TaskGraphManager &taskgraph_mgr, const Config &)
{
#ifdef MADRONA_GPU_MODE
    {
        TaskGraphBuilder &b = taskgraph_mgr.init(TaskGraphID::AppendOnly);
        b.addToGraph<ParallelForNode<Engine, appendSystem, StepCount>>({});
    }
    {
        TaskGraphBuilder &b = taskgraph_mgr.init(TaskGraphID::CompactOnly);
        b.addToGraph<CompactArchetypeNode<Body>>({});
    }
#endif
    TaskGraphBuilder &builder = taskgraph_mgr.init(TaskGraphID::Step);

    auto count = builder.addToGraph<ParallelForNode<Engine,
        countSystem, StepCount>>({});

    auto bvh = PhysicsSystem::setupBroadphaseTasks(builder, {count});
    auto step = PhysicsSystem::setupPhysicsStepTasks(
        builder, {bvh}, consts::numSubsteps);
    auto cleanup = PhysicsSystem::setupCleanupTasks(builder, {step});
    (void)cleanup;
}

static inline Quat randomRotation(RNG &rng)
{
    Vector3 axis {
        rng.sampleUniform() * 2.f - 1.f, rng.sampleUniform() * 2.f - 1.f,
        rng.sampleUniform() * 2.f - 1.f,
    };
    float angle = rng.sampleUniform() * 2.f;
    return Quat { 1.f, angle * axis.x, angle * axis.y, angle * axis.z }
        .normalize();
}

// the floor plane and four static wall cubes around [-half, half]^2
static inline void makePen(Engine &ctx, float half, float height)
{
    const Quat upright { 1, 0, 0, 0 };
    makeBody(ctx, Vector3 { 0.f, 0.f, 0.f }, upright, Diag3x3 { 1.f, 1.f, 1.f },
             SimObject::Plane, ResponseType::Static);
    const float thick = 0.5f;
    const float off = half + 0.5f * thick;
    const float len = 2.f * half + 2.f * thick;
    makeBody(ctx, Vector3 { -off, 0.f, 0.5f * height }, upright,
             Diag3x3 { thick, len, height }, SimObject::Cube, ResponseType::Static);
    makeBody(ctx, Vector3 { off, 0.f, 0.5f * height }, upright,
             Diag3x3 { thick, len, height }, SimObject::Cube, ResponseType::Static);
    makeBody(ctx, Vector3 { 0.f, -off, 0.5f * height }, upright,
             Diag3x3 { len, thick, height }, SimObject::Cube, ResponseType::Static);
    makeBody(ctx, Vector3 { 0.f, off, 0.5f * height }, upright,
             Diag3x3 { len, thick, height }, SimObject::Cube, ResponseType::Static);
}

Sim::Sim(Engine &ctx, const Config &cfg, const WorldInit &)
    : WorldBase(ctx)
{
    uint32_t global_world = cfg.worldBase + (uint32_t)ctx.worldID().idx;
    RandKey world_key = rand::split_i(rand::initKey(cfg.seed), global_world);
    RNG rng(world_key);

    ctx.singleton<StepCount>().n = 0;

    PhysicsSystem::init(ctx, cfg.rigidBodyObjMgr, consts::deltaT,
                        consts::numSubsteps, -9.8f * math::up, 128);

    const Quat upright { 1, 0, 0, 0 };
    if (global_world == consts::crowdedWorld) {
        // the crowded pen: a layer of small cubes on a grid and a smaller layer
        // on top of it, each cube a little into what it stands on, the outer
        // ones a little into the walls
        makePen(ctx, 3.1f, 2.f);
        const float pitch = 1.1f;
        const int32_t side = consts::crowdedSide;
        const float first = -0.5f * pitch * (float)(side - 1);
        float layer_z = 0.f;
        for (int32_t layer = 0; layer < consts::crowdedLayers; layer++) {
            const int32_t count = (side - layer) * (side - layer);
            for (int32_t i = 0; i < count; i++) {
                const float size = 0.6f + 0.2f * rng.sampleUniform();
                const float yaw = 0.3f * rng.sampleUniform() - 0.15f;
                makeBody(ctx,
                    Vector3 { first + pitch * (float)(i % side),
                              first + pitch * (float)(i / side),
                              layer_z + 0.29f },
                    Quat { 1.f, 0.f, 0.f, yaw }.normalize(),
                    Diag3x3 { size, size, 0.6f }, SimObject::Cube,
                    ResponseType::Dynamic);
            }
            layer_z += 0.59f;
        }
        // ... and a few that fall onto them
        for (int32_t i = 0; i < 4; i++) {
            makeBody(ctx,
                Vector3 { rng.sampleUniform() * 4.f - 2.f, rng.sampleUniform() * 4.f - 2.f,
                          2.5f + 1.2f * (float)i },
                randomRotation(rng), Diag3x3 { 0.7f, 0.7f, 0.7f }, SimObject::Cube,
                ResponseType::Dynamic);
        }
        return;
    }

    switch (global_world % 4u) {
    case 0: {
        // a pen: cubes of random shape and rotation dropped so that they stack
        makePen(ctx, 1.6f, 3.f);
        const int32_t num_cubes = 2 + (int32_t)(rng.sampleUniform() * 9.99f);
        for (int32_t i = 0; i < num_cubes; i++) {
            Entity e = makeBody(ctx,
                Vector3 { rng.sampleUniform() * 1.2f - 0.6f, rng.sampleUniform() * 1.2f - 0.6f,
                          1.4f + 2.6f * (float)i },
                randomRotation(rng),
                Diag3x3 { 0.6f + 1.2f * rng.sampleUniform(), 0.6f + 1.2f * rng.sampleUniform(),
                          0.6f + 1.2f * rng.sampleUniform() },
                SimObject::Cube, ResponseType::Dynamic);
            ctx.get<Velocity>(e).angular = Vector3 {
                rng.sampleUniform() * 2.f - 1.f, rng.sampleUniform() * 2.f - 1.f,
                rng.sampleUniform() * 2.f - 1.f,
            };
        }
    } break;
    case 1: {
        // a static slab and no plane: one sphere and a few cubes land on it
        makeBody(ctx, Vector3 { 0.f, 0.f, 0.f }, upright, Diag3x3 { 8.f, 8.f, 1.f },
                 SimObject::Cube, ResponseType::Static);
        makeBody(ctx,
            Vector3 { rng.sampleUniform() - 0.5f, rng.sampleUniform() - 0.5f, 1.3f },
            upright, Diag3x3 { 1.f, 1.f, 1.f }, SimObject::Sphere, ResponseType::Dynamic);
        const int32_t num_cubes = 2 + (int32_t)(rng.sampleUniform() * 2.99f);
        for (int32_t i = 0; i < num_cubes; i++) {
            makeBody(ctx,
                Vector3 { rng.sampleUniform() * 1.6f - 0.8f, rng.sampleUniform() * 1.6f - 0.8f,
                          2.6f + 1.8f * (float)i },
                randomRotation(rng),
                Diag3x3 { 0.6f + 0.8f * rng.sampleUniform(), 0.6f + 0.8f * rng.sampleUniform(),
                          0.6f + 0.8f * rng.sampleUniform() },
                SimObject::Cube, ResponseType::Dynamic);
        }
    } break;
    case 2: {
        // statics only, one into the other: bodies, and no pair that counts
        makeBody(ctx, Vector3 { 0.f, 0.f, 0.f }, upright, Diag3x3 { 1.f, 1.f, 1.f },
                 SimObject::Plane, ResponseType::Static);
        for (int32_t i = 0; i < 3; i++) {
            makeBody(ctx, Vector3 { 0.4f * (float)i, 0.f, 0.3f }, randomRotation(rng),
                     Diag3x3 { 1.f, 1.f, 1.f }, SimObject::Cube, ResponseType::Static);
        }
    } break;
    default:
        // no bodies at all
        break;
    }
}

#ifdef MADRONA_GPU_MODE
MADRONA_BUILD_MWGPU_ENTRY(Engine, Sim, Sim::Config, Sim::WorldInit);
#endif

}
