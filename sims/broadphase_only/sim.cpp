#include "sim.hpp"

#ifdef MADRONA_GPU_MODE
#include <madrona/mw_gpu_entry.hpp>
#endif

using namespace madrona;
using namespace madrona::math;
using namespace madrona::phys;
using madrona::base::Rotation;
using madrona::base::Scale;
using madrona::base::ObjectID;

namespace bponly {

void Sim::registerTypes(ECSRegistry &registry, const Config &cfg)
{
    base::registerTypes(registry);
    PhysicsSystem::registerTypes(registry);

    registry.registerComponent<Drift>();
    registry.registerComponent<RayFan>();
    registry.registerComponent<RayFanPlain>();
    registry.registerComponent<Probe32>();
    registry.registerComponent<Probe64>();
    registry.registerSingleton<StepCount>();

    registry.registerArchetype<Box>();
    registry.registerArchetype<Pillar>();
    registry.registerArchetype<Sensor>();
    registry.registerArchetype<Prober>();

    registry.exportSingleton<StepCount>((uint32_t)ExportID::StepCount);
    if ((cfg.flags & plan::flagExportPosition) != 0) {
        registry.exportColumn<Box, Position>((uint32_t)ExportID::BoxPosition);
    }
}

static inline void setupBody(Engine &ctx, Entity e, Vector3 pos, Diag3x3 scale,
                             ResponseType response)
{
    ObjectID obj_id { 0 };
    ctx.get<Position>(e) = pos;
    ctx.get<Rotation>(e) = Quat { 1, 0, 0, 0 };
    ctx.get<Scale>(e) = scale;
    ctx.get<ObjectID>(e) = obj_id;
    ctx.get<ResponseType>(e) = response;
    ctx.get<Velocity>(e) = Velocity { Vector3::zero(), Vector3::zero() };
    ctx.get<ExternalForce>(e) = Vector3::zero();
    ctx.get<ExternalTorque>(e) = Vector3::zero();
    ctx.get<broadphase::LeafID>(e) =
        PhysicsSystem::registerEntity(ctx, e, obj_id);
}

inline void driftSystem(Engine &,
                        Position &pos,
                        Velocity &vel,
                        Drift &drift)
{
    Vector3 p = pos;
    Vector3 v = drift.v;

    // (a still body stays where it was put, outside the arena too: the still
    // layouts of plan mode)
    if (v.x == 0.f && v.y == 0.f) {
        return;
    }

    p += consts::deltaT * v;
    if (p.x < -consts::arena) { p.x = -consts::arena; v.x = -v.x; }
    if (p.x > consts::arena) { p.x = consts::arena; v.x = -v.x; }
    if (p.y < -consts::arena) { p.y = -consts::arena; v.y = -v.y; }
    if (p.y > consts::arena) { p.y = consts::arena; v.y = -v.y; }

    pos = p;
    drift.v = v;
    vel.linear = v;    // the BVH sweeps leaf boxes along the velocity
}

// every rebuildPeriod steps the world empties its BVH and registers its bodies
// again (in a different order): the tree is rebuilt on the next update
inline void reregisterSystem(Engine &ctx, StepCount &steps)
{
    Sim &sim = ctx.data();

    steps.n += 1;
    if (steps.n % sim.rebuildPeriod != 0) {
        return;
    }

    PhysicsSystem::reset(ctx);
    for (int32_t i = sim.numBoxes - 1; i >= 0; i--) {
        Entity e = sim.boxes[i];
        ctx.get<broadphase::LeafID>(e) =
            PhysicsSystem::registerEntity(ctx, e, ctx.get<ObjectID>(e));
    }
    for (int32_t i = 0; i < sim.numPillars; i++) {
        Entity e = sim.pillars[i];
        ctx.get<broadphase::LeafID>(e) =
            PhysicsSystem::registerEntity(ctx, e, ctx.get<ObjectID>(e));
    }
}

// (plan::flagCarriedNudge) moves the world's first box without telling anyone
inline void nudgeSystem(Engine &ctx, StepCount &)
{
    Sim &sim = ctx.data();
    if (sim.numBoxes > 0) {
        Vector3 p = ctx.get<Position>(sim.boxes[0]);
        p.z += 0.125f;
        ctx.get<Position>(sim.boxes[0]) = p;
    }
}

// sensors drift like the boxes (no body: they are not in the BVH)
inline void sensorDriftSystem(Engine &, Position &pos, Drift &drift, RayFan &)
{
    Vector3 p = pos;
    Vector3 v = drift.v;
    p += consts::deltaT * v;
    if (p.x < -consts::arena) { p.x = -consts::arena; v.x = -v.x; }
    if (p.x > consts::arena) { p.x = consts::arena; v.x = -v.x; }
    if (p.y < -consts::arena) { p.y = -consts::arena; v.y = -v.y; }
    if (p.y > consts::arena) { p.y = consts::arena; v.y = -v.y; }
    pos = p;
    drift.v = v;
}

// Ray i of the fan: a fan in the plane plus a tilt that differs per ray, so
// that rays leave through tops and sides of the boxes.  Plan mode replaces the
// first five by the axis-aligned +x, -x, +y, -y, -z (zero components: slabs the
// ray runs parallel to).
static inline Vector3 fanDirection(int32_t i, bool plan_mode)
{
    if (plan_mode && i < 5) {
        const float s = (i & 1) ? -1.f : 1.f;
        if (i < 2) return Vector3 { s, 0.f, 0.f };
        if (i < 4) return Vector3 { 0.f, s, 0.f };
        return Vector3 { 0.f, 0.f, -1.f };
    }
    // (directions from integers: no transcendental functions, whose last
    // bit differs between libm and the device library)
    return Vector3 {
        (float)((i * 7) % 11 - 5) + 0.5f,
        (float)((i * 3) % 13 - 6) + 0.25f,
        0.75f * (float)((i % 5) - 2) }.normalize();
}

// 32 rays from the sensor's position
inline void raySystem(Engine &ctx, const Position &pos, RayFan &fan)
{
    broadphase::BVH &bvh = ctx.singleton<broadphase::BVH>();
    Vector3 ray_o = pos;
    const bool plan_mode = (ctx.data().flags & plan::flagPlan) != 0;

#if defined(MADRONA_GPU_MODE) && !defined(SIM_PORTABLE)
    broadphase::BVH::RayGroupScratch *ray_scratch = broadphase::rayGroupScratch();
#endif
    auto trace = [&](int32_t i) {
        Vector3 ray_d = fanDirection(i, plan_mode);
        float hit_t;
        Vector3 hit_normal;
#if defined(MADRONA_GPU_MODE) && !defined(SIM_PORTABLE)
        Entity hit = bvh.traceRayShared(ray_scratch, ray_o, ray_d, &hit_t,
                                        &hit_normal, 40.f);
#else
        Entity hit = bvh.traceRay(ray_o, ray_d, &hit_t, &hit_normal, 40.f);
#endif
        if (hit == Entity::none()) {
            fan.hitT[i] = 0.f;
            fan.hitEntity[i] = -1;
            fan.hitNormal[i] = Vector3::zero();
        } else {
            fan.hitT[i] = hit_t;
            fan.hitEntity[i] = hit.id;
            fan.hitNormal[i] = hit_normal;
        }
    };

#ifdef MADRONA_GPU_MODE
    trace((int32_t)(threadIdx.x % 32));
#else
    for (int32_t i = 0; i < consts::raysPerSensor; i++) {
        trace(i);
    }
#endif
}

// (plan mode) plan::plainRayIndex's rays of the fan once more through plain
// BVH::traceRay, a lane per sensor on every backend: traceRay and
// traceRayShared are diffed against the reference on the same trees
inline void plainRaySystem(Engine &ctx, const Position &pos, RayFanPlain &fan)
{
    broadphase::BVH &bvh = ctx.singleton<broadphase::BVH>();
    Vector3 ray_o = pos;

    for (int32_t k = 0; k < consts::plainRays; k++) {
        Vector3 ray_d = fanDirection(plan::plainRayIndex(k), true);
        float hit_t;
        Vector3 hit_normal;
        Entity hit = bvh.traceRay(ray_o, ray_d, &hit_t, &hit_normal, 40.f);
        if (hit == Entity::none()) {
            fan.hitT[k] = 0.f;
            fan.hitEntity[k] = -1;
            fan.hitNormal[k] = Vector3::zero();
        } else {
            fan.hitT[k] = hit_t;
            fan.hitEntity[k] = hit.id;
            fan.hitNormal[k] = hit_normal;
        }
    }
}

// (plan mode) four query boxes per world: around its first box (half extent
// 0.4), its first sensor (1), its last sensor (3) and its first sensor again
// (50: contains everything).  The first DYNAMIC entity in each: the static
// pillars are visited and skipped.
template <int LANES>
static inline void probeWorld(Engine &ctx, int32_t *found_out)
{
    const Sim &sim = ctx.data();

    Vector3 centres[consts::numProbeBoxes];
    centres[0] = sim.numBoxes > 0 ?
        (Vector3)ctx.get<Position>(sim.boxes[0]) : Vector3::zero();
    centres[1] = ctx.get<Position>(sim.sensors[0]);
    centres[2] = ctx.get<Position>(sim.sensors[sim.numSensors - 1]);
    centres[3] = centres[1];

    math::AABB boxes[consts::numProbeBoxes];
    for (int32_t k = 0; k < consts::numProbeBoxes; k++) {
        const float half = plan::probeHalf(k);
        boxes[k] = math::AABB {
            .pMin = centres[k] - Vector3 { half, half, half },
            .pMax = centres[k] + Vector3 { half, half, half },
        };
    }
    auto accept = [&](Entity e) {
        return ctx.get<ResponseType>(e) == ResponseType::Dynamic;
    };

    Entity first[consts::numProbeBoxes];
#ifdef MADRONA_GPU_MODE
    // (CustomParallelForNode<..., LANES, 1, ...>: LANES lanes per world)
    PhysicsSystem::findFirstEntitiesWithinAABBsWave<consts::numProbeBoxes, LANES>(
        ctx, boxes, consts::numProbeBoxes, first, accept);
    if (threadIdx.x % LANES != 0) {
        return;
    }
#else
    for (int32_t k = 0; k < consts::numProbeBoxes; k++) {
        first[k] = Entity::none();
        PhysicsSystem::findEntitiesWithinAABB(ctx, boxes[k], [&](Entity e) {
            if (first[k] == Entity::none() && accept(e)) {
                first[k] = e;
            }
        });
    }
#endif

    for (int32_t k = 0; k < consts::numProbeBoxes; k++) {
        found_out[k] = first[k] == Entity::none() ? -1 : first[k].id;
    }
}

inline void probe32System(Engine &ctx, Probe32 &probe)
{
    probeWorld<32>(ctx, probe.found);
}

inline void probe64System(Engine &ctx, Probe64 &probe)
{
    probeWorld<64>(ctx, probe.found);
}

void Sim::setupTasks(TaskGraphManager &taskgraph_mgr, const Config &cfg)
{
    TaskGraphBuilder &builder = taskgraph_mgr.init(0);

    // last step's pairs stay readable until the next step starts
    auto cleanup =
        PhysicsSystem::setupStandaloneBroadphaseCleanupTasks(builder, {});

#if defined(MADRONA_GPU_MODE) && !defined(SIM_PORTABLE)
    if ((cfg.flags & plan::flagCarried) != 0) {
        if ((cfg.flags & plan::flagCarriedNudge) != 0) {
            cleanup = builder.addToGraph<ParallelForNode<Engine,
                nudgeSystem, StepCount>>({cleanup});
        }
        cleanup = PhysicsSystem::setupBroadphaseTasks(builder, {cleanup},
            PhysicsSystem::BroadphaseInputs::CarriedOver);
    }
#endif

    auto drift = builder.addToGraph<ParallelForNode<Engine,
        driftSystem, Position, Velocity, Drift>>({cleanup});

    auto reregister = builder.addToGraph<ParallelForNode<Engine,
        reregisterSystem, StepCount>>({drift});

    auto bvh = PhysicsSystem::setupBroadphaseTasks(builder, {reregister});

    const bool plan_mode = (cfg.flags & plan::flagPlan) != 0;
    if ((cfg.flags & plan::flagRays) != 0 || plan_mode) {
        auto sensor_drift = builder.addToGraph<ParallelForNode<Engine,
            sensorDriftSystem, Position, Drift, RayFan>>({bvh});
#ifdef MADRONA_GPU_MODE
        bvh = builder.addToGraph<CustomParallelForNode<Engine,
            raySystem, 32, 1, Position, RayFan>>({sensor_drift});
#else
        bvh = builder.addToGraph<ParallelForNode<Engine,
            raySystem, Position, RayFan>>({sensor_drift});
#endif
    }

    if (plan_mode) {
        bvh = builder.addToGraph<ParallelForNode<Engine,
            plainRaySystem, Position, RayFanPlain>>({bvh});
#ifdef MADRONA_GPU_MODE
        bvh = builder.addToGraph<CustomParallelForNode<Engine,
            probe32System, 32, 1, Probe32>>({bvh});
        bvh = builder.addToGraph<CustomParallelForNode<Engine,
            probe64System, 64, 1, Probe64>>({bvh});
#else
        bvh = builder.addToGraph<ParallelForNode<Engine,
            probe32System, Probe32>>({bvh});
        bvh = builder.addToGraph<ParallelForNode<Engine,
            probe64System, Probe64>>({bvh});
#endif
    }

    auto overlaps =
        PhysicsSystem::setupStandaloneBroadphaseOverlapTasks(builder, {bvh});

#ifdef MADRONA_GPU_MODE
    // group the pairs by world (stable) so they can be read per world
    overlaps = builder.addToGraph<
        SortArchetypeNode<CandidateTemporary, WorldID>>({overlaps});
#endif
    (void)overlaps;
}

Sim::Sim(Engine &ctx, const Config &cfg, const WorldInit &)
    : WorldBase(ctx)
{
    uint32_t global_world = cfg.worldBase + (uint32_t)ctx.worldID().idx;
    RNG rng(rand::split_i(rand::initKey(cfg.seed), global_world));

    ctx.singleton<StepCount>().n = 0;

    flags = cfg.flags;
    numSensors = 0;
    if ((cfg.flags & plan::flagPlan) != 0) {
        initPlanWorld(ctx, cfg, global_world, rng);
        return;
    }

    const bool ray_mode = (cfg.flags & plan::flagRays) != 0;
    // (ray mode: 10 .. 100 boxes, by the global world index)
    numBoxes = ray_mode ?
        10 + (int32_t)((global_world * 37u) % 91u) : consts::numBoxes;
    numPillars = consts::numPillars;
    rebuildPeriod = consts::rebuildPeriod;

    PhysicsSystem::init(ctx, cfg.rigidBodyObjMgr, consts::deltaT, 1,
                        -9.8f * math::up,
                        ray_mode ?
                            consts::rayModeMaxBoxes + consts::numPillars : 32);

    for (int32_t i = 0; i < consts::numPillars; i++) {
        pillars[i] = ctx.makeEntity<Pillar>();
        setupBody(ctx, pillars[i],
            Vector3 { (i & 1) ? 2.5f : -2.5f, (i & 2) ? 2.5f : -2.5f, 1.f },
            Diag3x3 { 1.f, 1.f, 2.f }, ResponseType::Static);
    }

    for (int32_t i = 0; i < numBoxes; i++) {
        makeDriftingBox(ctx, rng, i);
    }

    if (ray_mode) {
        const int32_t num_sensors = 1 + (int32_t)(global_world % 3u);
        for (int32_t i = 0; i < num_sensors; i++) {
            makeSensor(ctx, rng);
        }
    }
}

void Sim::makeDriftingBox(Engine &ctx, RNG &rng, int32_t i)
{
    boxes[i] = ctx.makeEntity<Box>();
    float size = 0.6f + rng.sampleUniform();
    setupBody(ctx, boxes[i],
        Vector3 {
            (rng.sampleUniform() * 2.f - 1.f) * consts::arena,
            (rng.sampleUniform() * 2.f - 1.f) * consts::arena,
            size * 0.5f,
        },
        Diag3x3 { size, size, size }, ResponseType::Dynamic);
    ctx.get<Drift>(boxes[i]).v = Vector3 {
        rng.sampleUniform() * 4.f - 2.f, rng.sampleUniform() * 4.f - 2.f, 0.f,
    };
}

// a sensor at a random place of the arena, drifting
Entity Sim::makeSensor(Engine &ctx, RNG &rng)
{
    Entity e = ctx.makeEntity<Sensor>();
    ctx.get<Position>(e) = Vector3 {
        (rng.sampleUniform() * 2.f - 1.f) * consts::arena,
        (rng.sampleUniform() * 2.f - 1.f) * consts::arena,
        0.3f + rng.sampleUniform(),
    };
    ctx.get<Drift>(e).v = Vector3 {
        rng.sampleUniform() * 3.f - 1.5f, rng.sampleUniform() * 3.f - 1.5f,
        0.f,
    };
    RayFan &fan = ctx.get<RayFan>(e);
    for (int32_t r = 0; r < consts::raysPerSensor; r++) {
        fan.hitT[r] = 0.f;
        fan.hitEntity[r] = -1;
        fan.hitNormal[r] = Vector3::zero();
    }
    RayFanPlain &plain = ctx.get<RayFanPlain>(e);
    for (int32_t r = 0; r < consts::plainRays; r++) {
        plain.hitT[r] = 0.f;
        plain.hitEntity[r] = -1;
        plain.hitNormal[r] = Vector3::zero();
    }
    sensors[numSensors++] = e;
    return e;
}

// Plan mode (sim.hpp): everything from the global world index and the flags.
void Sim::initPlanWorld(Engine &ctx, const Config &cfg, uint32_t global_world,
                        RNG &rng)
{
    using plan::Layout;
    using plan::MaxLeaves;

    const int32_t num_leaves = plan::leafCount(global_world);
    const bool no_pillars = (cfg.flags & plan::flagNoPillars) != 0;
    numPillars = (num_leaves >= plan::pillarMinLeaves && !no_pillars) ?
        consts::numPillars : 0;
    numBoxes = num_leaves - numPillars;
    rebuildPeriod = consts::planRebuildPeriod;

    Layout layout = (Layout)((cfg.flags >> plan::layoutShift) & 7u);
    MaxLeaves max_mode = (MaxLeaves)((cfg.flags >> plan::maxLeavesShift) & 3u);
    if (layout == Layout::Doubling) {
        if (num_leaves <= plan::doublingMaxLeaves) {
            max_mode = MaxLeaves::Staged64;
        } else {
            layout = Layout::Line;
        }
    }

    int32_t max_leaves = num_leaves > 1 ? num_leaves : 1;
    if (num_leaves <= 64 && max_mode == MaxLeaves::Staged64) {
        max_leaves = 64;
    } else if (num_leaves <= 64 && max_mode == MaxLeaves::InPlace65) {
        max_leaves = 65;
    }

    PhysicsSystem::init(ctx, cfg.rigidBodyObjMgr, consts::deltaT, 1,
                        -9.8f * math::up, max_leaves);

    for (int32_t i = 0; i < numPillars; i++) {
        pillars[i] = ctx.makeEntity<Pillar>();
        setupBody(ctx, pillars[i],
            Vector3 { (i & 1) ? 2.5f : -2.5f, (i & 2) ? 2.5f : -2.5f, 1.f },
            Diag3x3 { 1.f, 1.f, 2.f }, ResponseType::Static);
    }

    // still layouts: zero drift (leaf boxes symmetric about the body, so equal
    // inputs give bit-equal centres), coordinates exact in binary
    int32_t lattice_k = 1;
    while (lattice_k * lattice_k < numBoxes) {
        lattice_k++;
    }
    for (int32_t i = 0; i < numBoxes; i++) {
        if (layout == Layout::Drift) {
            makeDriftingBox(ctx, rng, i);
            continue;
        }

        Vector3 pos { 0.5f, -0.25f, 0.5f };
        float size = 1.f;
        switch (layout) {
        case Layout::Line: {
            size = 0.5f;
            pos = Vector3 { -4.5f + 0.0625f * (float)i, 0.25f, 0.25f };
        } break;
        case Layout::Lattice: {
            // the diagonal first (equal x and y extents from k boxes on), then
            // the other cells row by row
            int32_t cx = i, cy = i;
            if (i >= lattice_k) {
                int32_t cell = i - lattice_k;       // among the off-diagonal cells
                cy = cell / (lattice_k - 1);
                cx = cell % (lattice_k - 1);
                if (cx >= cy) cx++;
            }
            size = 0.5f;
            pos = Vector3 { -2.25f + 0.375f * (float)cx,
                            -2.25f + 0.375f * (float)cy, 0.25f };
        } break;
        case Layout::Outlier: {
            if (i == numBoxes - 1 && numBoxes > 1) {
                pos.x = 30.5f;
            }
        } break;
        case Layout::Nested: {
            size = 0.5f + 0.0625f * (float)i;
            pos = Vector3 { 0.f, 0.5f, 5.f };
        } break;
        case Layout::Doubling: {
            size = 0.5f;
            pos = Vector3 { (float)(1u << i) * 0.015625f, 0.f, 0.25f };
        } break;
        default: break;     // Coincident
        }

        boxes[i] = ctx.makeEntity<Box>();
        setupBody(ctx, boxes[i], pos, Diag3x3 { size, size, size },
                  ResponseType::Dynamic);
        ctx.get<Drift>(boxes[i]).v = Vector3::zero();
    }

    // 1 .. 3 sensors; the first one hangs still above the first box, inside its
    // footprint (its -z ray meets the box: every world with a leaf sees hits)
    const int32_t num_sensors = 1 + (int32_t)(global_world % 3u);
    for (int32_t i = 0; i < num_sensors; i++) {
        Entity e = makeSensor(ctx, rng);
        if (i == 0 && numBoxes > 0) {
            const Vector3 box_pos = ctx.get<Position>(boxes[0]);
            const float box_size = ctx.get<Scale>(boxes[0]).d0;
            const float dx = (rng.sampleUniform() - 0.5f) * 0.6f * box_size;
            const float dy = (rng.sampleUniform() - 0.5f) * 0.6f * box_size;
            const float dz = 0.25f + 0.5f * rng.sampleUniform();
            ctx.get<Position>(e) = Vector3 {
                box_pos.x + dx, box_pos.y + dy,
                box_pos.z + 0.5f * box_size + dz,
            };
            ctx.get<Drift>(e).v = Vector3::zero();
        }
    }

    Entity prober = ctx.makeEntity<Prober>();
    for (int32_t k = 0; k < consts::numProbeBoxes; k++) {
        ctx.get<Probe32>(prober).found[k] = -1;
        ctx.get<Probe64>(prober).found[k] = -1;
    }
}

#ifdef MADRONA_GPU_MODE
MADRONA_BUILD_MWGPU_ENTRY(Engine, Sim, Sim::Config, Sim::WorldInit);
#endif

}
