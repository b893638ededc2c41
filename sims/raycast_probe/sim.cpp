#include "sim.hpp"

#ifdef MADRONA_GPU_MODE
#include <madrona/mw_gpu_entry.hpp>
#endif

using namespace madrona;
using namespace madrona::math;
using namespace madrona::render;

namespace raycastprobe {

void Sim::registerTypes(ECSRegistry &registry, const Config &cfg)
{
    base::registerTypes(registry);
    RenderingSystem::registerTypes(registry, cfg.bridge);

    registry.registerSingleton<StepCount>();

    registry.registerArchetype<Thing>();
    registry.registerArchetype<Viewer>();
    registry.registerArchetype<Lamp>();

    registry.exportSingleton<StepCount>((uint32_t)ExportID::Steps);
#ifdef MADRONA_GPU_MODE
    registry.exportColumn<RaycastOutputArchetype, RGBOutputBuffer>(
        (uint32_t)ExportID::RGB);
    registry.exportColumn<RaycastOutputArchetype, DepthOutputBuffer>(
        (uint32_t)ExportID::Depth);
#endif
}

namespace {

enum : int32_t { Box = 0, Ellipsoid = 1, Cylinder = 2, Wedge = 3, Sheared = 4 };

constexpr int32_t kDefault = MaterialOverride::UseDefaultMaterial;
constexpr int32_t kColor = MaterialOverride::UseOverrideColor;
// materials only ever reached through MaterialOverride (mgr.cpp): a plain one
// and a textured one
constexpr int32_t kPlainOverride = 3;
constexpr int32_t kTexturedOverride = 7;

// (no trigonometry: both backends must agree to the bit)
inline Quat quat(float w, float x, float y, float z)
{
    return Quat { w, x, y, z }.normalize();
}

void place(Engine &ctx, int32_t object, Vector3 pos, Quat rot, Diag3x3 scale,
           int32_t mat = kDefault, uint32_t color = 0u)
{
    Entity e = ctx.makeEntity<Thing>();
    ctx.get<Position>(e) = pos;
    ctx.get<Rotation>(e) = rot;
    ctx.get<Scale>(e) = scale;
    ctx.get<ObjectID>(e) = ObjectID { object };
    ctx.get<MaterialOverride>(e).matID = mat;
    ctx.get<ColorOverride>(e).color = 0xFF000000u | color;
    RenderingSystem::makeEntityRenderable(ctx, e);
}

void light(Engine &ctx, bool directional, Vector3 pos, Vector3 dir,
           float cutoff, bool shadow)
{
    Entity e = ctx.makeEntity<Lamp>();
    ctx.get<Position>(e) = pos;
    ctx.get<LightDescDirection>(e) = LightDescDirection(dir);
    ctx.get<LightDescType>(e).type =
        directional ? LightDesc::Directional : LightDesc::Spotlight;
    ctx.get<LightDescShadow>(e).castShadow = shadow;
    ctx.get<LightDescCutoffAngle>(e).cutoff = cutoff;
    ctx.get<LightDescIntensity>(e).intensity = 1.f;
    ctx.get<LightDescActive>(e).active = true;
    RenderingSystem::makeEntityLightCarrier(ctx, e);
}

void sun(Engine &ctx, Vector3 dir, bool shadow = false)
{
    light(ctx, true, Vector3 { 0.f, 0.f, 20.f }, dir, -1.f, shadow);
}

// the light most kinds have: from behind the cameras, from the left and above
inline Vector3 sunDir() { return Vector3 { 0.3f, 0.8f, -0.5f }; }

// a rotation no axis of which is a coordinate axis
inline Quat tilted() { return quat(1.f, 0.3f, 0.2f, 0.4f); }

// kinds 3 and 11: one instance of each mesh
void everyMesh(Engine &ctx)
{
    place(ctx, Box, Vector3 { -4.5f, 8.f, 1.5f }, quat(1.f, 0.1f, 0.05f, 0.15f),
          Diag3x3 { 3.f, 2.f, 3.5f }, kColor, 0x20C0A0u);
    place(ctx, Ellipsoid, Vector3 { -1.6f, 6.f, 0.2f }, tilted(),
          Diag3x3 { 1.6f, 2.5f, 1.8f });
    place(ctx, Cylinder, Vector3 { 1.2f, 5.f, 2.6f }, quat(1.f, 0.5f, 0.1f, 0.2f),
          Diag3x3 { 1.6f, 1.3f, 4.f }, kPlainOverride);
    // default material: its triangles carry theirs, two of them textured
    place(ctx, Wedge, Vector3 { 1.5f, 6.f, -1.5f }, quat(1.f, 0.6f, -0.2f, 0.3f),
          Diag3x3 { 2.5f, 3.f, 4.f });
    // a textured material by override: sampled at the mesh's own uvs
    place(ctx, Sheared, Vector3 { 4.f, 7.f, 2.f }, quat(1.f, -0.2f, 0.3f, -0.25f),
          Diag3x3 { 2.5f, 1.5f, 3.f }, kTexturedOverride);
}

// kinds 4, 5, 6: a wall of `total - 1` small objects in front of a slab
void wall(Engine &ctx, int32_t total)
{
    for (int32_t i = 0; i < total - 1; i++) {
        const Vector3 pos { -4.8f + 0.8f * (float)(i % 13), 7.f + 0.45f * (float)(i % 3),
                            -0.1f + 0.8f * (float)(i / 13) };
        if (i == 5) {
            place(ctx, Ellipsoid, pos, tilted(), Diag3x3 { 0.3f, 0.9f, 0.25f });
        } else if (i == 20) {
            place(ctx, Sheared, pos, quat(1.f, 0.2f, -0.3f, 0.1f),
                  Diag3x3 { 0.4f, 0.5f, 0.6f });
        } else if (i == 40) {
            place(ctx, Wedge, pos, quat(1.f, 0.7f, 0.2f, -0.1f),
                  Diag3x3 { 0.4f, 0.6f, 0.9f });
        } else {
            place(ctx, Box, pos, quat(1.f, 0.f, 0.f, 0.02f * (float)(i % 7)),
                  Diag3x3 { 0.5f, 0.4f + 0.05f * (float)(i % 4), 0.5f },
                  i % 4 == 0 ? kColor : kDefault, (uint32_t)(i * 197003));
        }
    }
    place(ctx, Box, Vector3 { 0.f, 9.5f, 1.5f }, Quat { 1.f, 0.f, 0.f, 0.f },
          Diag3x3 { 14.f, 0.5f, 7.f }, kPlainOverride);
    sun(ctx, Vector3 { 0.55f, 0.7f, -0.35f }, true);
}

// kind 8: all within 1e-3 of one point, the low mantissa bits of the
// coordinates chosen so that the sorted Morton codes are the pairs
// (1 << (29 - k)) | {0, 1}: every level of the Karras tree splits one pair off
// the rest, both children internal nodes.  Bars through the common point,
// fanned out about the view axis (no two of the same depth: no coplanar
// faces), the innermost ones ellipsoids; a slab through all of them catches
// their shadows.
void deepTree(Engine &ctx, int32_t pairs)
{
    // (a code takes bits 0-9 of a coordinate's pattern, bits 8 and 9 ORed with
    // bits 24 and 25 -- two exponent bits: clear in [2, 8) and in [2^-7, 2^-5))
    const uint32_t base[3] = { __builtin_bit_cast(uint32_t, 0.0078125f),
                               __builtin_bit_cast(uint32_t, 6.f),
                               __builtin_bit_cast(uint32_t, 2.f) };
    const int32_t n = 2 * pairs;
    for (int32_t k = 0; k < pairs; k++) {
        const int32_t bit = 29 - k;
        for (int32_t odd = 0; odd < 2; odd++) {
            uint32_t bits[3] = { base[0], base[1], base[2] };
            bits[bit % 3] |= 1u << (bit / 3);
            bits[0] |= (uint32_t)odd;
            const Vector3 pos { __builtin_bit_cast(float, bits[0]),
                                __builtin_bit_cast(float, bits[1]),
                                __builtin_bit_cast(float, bits[2]) };
            const int32_t m = 2 * k + odd;
            // tan of half the angle about the view axis
            const float t = -1.f + 2.f * (float)m / (float)n;
            if (m == 0) {
                place(ctx, Box, pos, Quat { 1.f, 0.f, 0.f, 0.f },
                      Diag3x3 { 11.f, 0.5f, 8.f }, kPlainOverride);
            } else if (k >= pairs - 3) {
                // (turned half round: the mesh lies on the +z side of its origin)
                place(ctx, Ellipsoid, pos, quat(t, 0.05f, 1.f, 0.03f),
                      Diag3x3 { 3.f, 3.f + 0.07f * (float)m, 0.8f });
            } else {
                place(ctx, Box, pos, quat(1.f, 0.f, t, 0.f),
                      Diag3x3 { 7.f, 1.f + 0.06f * (float)m, 1.7f },
                      m % 3 == 0 ? kColor : kDefault, (uint32_t)(m * 461939));
            }
        }
    }
    // More than the 64 instances the ray caster stages per world, so that
    // primary rays walk the top-level tree as well (shadow rays always do):
    // thin bars at the same point whose codes, (3 << 28) | j, join the tree next
    // to the root and leave the chain as it is.
    for (int32_t j = 2; j < 2 + consts::deepFillers; j++) {
        uint32_t bits[3] = { base[0], base[1] | (1u << 9), base[2] | (1u << 9) };
        for (int32_t b = 0; b < 6; b++) {
            bits[b % 3] |= (((uint32_t)j >> b) & 1u) << (b / 3);
        }
        const Vector3 pos { __builtin_bit_cast(float, bits[0]),
                            __builtin_bit_cast(float, bits[1]),
                            __builtin_bit_cast(float, bits[2]) };
        const float t = -0.97f + 2.f * (float)(j - 2) / (float)consts::deepFillers;
        place(ctx, Box, pos, quat(1.f, 0.f, t, 0.f),
              Diag3x3 { 9.f, 0.7f + 0.007f * (float)j, 0.2f }, kColor,
              (uint32_t)(j * 318211));
    }
    sun(ctx, Vector3 { 0.45f, 0.8f, -0.4f }, true);
}

}

inline void tickSystem(Engine &, StepCount &count)
{
    count.steps += 1;
}

void Sim::setupTasks(TaskGraphManager &taskgraph_mgr, const Config &)
{
    TaskGraphBuilder &builder = taskgraph_mgr.init(0);

    auto tick = builder.addToGraph<ParallelForNode<Engine,
        tickSystem, StepCount>>({});

    RenderingSystem::setupTasks(builder, {tick}, true);
}

Sim::Sim(Engine &ctx, const Config &cfg, const WorldInit &)
    : WorldBase(ctx)
{
    const uint32_t global_world = cfg.worldBase + (uint32_t)ctx.worldID().idx;
    kind = (int32_t)(global_world % (uint32_t)consts::numKinds);
    ctx.singleton<StepCount>().steps = 0;

    RenderingSystem::init(ctx, cfg.bridge);

    const Quat upright { 1.f, 0.f, 0.f, 0.f };

    switch (kind) {
    case 0:
        sun(ctx, sunDir());
        break;
    case 1:
        place(ctx, Box, Vector3 { 0.3f, 7.f, 1.6f }, quat(1.f, 0.1f, 0.05f, 0.15f),
              Diag3x3 { 6.f, 2.f, 5.f });
        sun(ctx, sunDir());
        break;
    case 2:
        place(ctx, Box, Vector3 { 0.1f, 9.1f, 1.45f }, upright,
              Diag3x3 { 9.f, 1.f, 6.f });
        place(ctx, Ellipsoid, Vector3 { 0.2f, 5.f, 0.3f }, tilted(),
              Diag3x3 { 1.5f, 2.5f, 1.5f });
        sun(ctx, sunDir());
        break;
    case 3:
        everyMesh(ctx);
        sun(ctx, sunDir());
        break;
    case 4: case 5: case 6:
        wall(ctx, 59 + kind);
        break;
    case 7:
        // one and the same position: equal Morton codes; bars fanned out about
        // the view axis, so that each pokes out of the others
        for (int32_t i = 0; i < 17; i++) {
            const float t = 0.12f * (float)(i - 8) + 0.03f;
            const Vector3 pos { 0.7f, 7.f, 1.8f };
            if (i % 5 == 0) {
                place(ctx, Box, pos, quat(1.f, 0.f, t, 0.f),
                      Diag3x3 { 9.f, 1.f + 0.1f * (float)i, 1.f },
                      i == 10 ? kColor : kDefault, 0xE0E020u);
            } else {
                place(ctx, i % 5, pos, quat(1.f, 0.07f, t, 0.05f),
                      Diag3x3 { 5.f + 0.3f * (float)i, 2.f, 1.5f },
                      i % 5 == Sheared ? kTexturedOverride : kDefault);
            }
        }
        sun(ctx, sunDir());
        break;
    case 8:
        deepTree(ctx, cfg.tooDeep != 0u ? consts::tooDeepPairs : consts::deepPairs);
        break;
    case 9:
        // viewer 0 sits inside this box: all of its faces are back faces
        place(ctx, Box, Vector3 { 0.f, 0.f, 1.5f }, upright,
              Diag3x3 { 2.f, 2.f, 2.f });
        place(ctx, Ellipsoid, Vector3 { -1.5f, 6.f, 0.5f }, tilted(),
              Diag3x3 { 2.f, 3.f, 2.f });
        place(ctx, Box, Vector3 { 2.5f, 7.f, 2.f }, quat(1.f, 0.1f, 0.2f, 0.3f),
              Diag3x3 { 3.f, 2.f, 3.f }, kColor, 0xC04040u);
        // wholly behind both cameras
        place(ctx, Sheared, Vector3 { 0.5f, -8.f, 1.5f }, tilted(),
              Diag3x3 { 3.f, 2.f, 4.f });
        // the floor: in front of the cameras, under them and behind them
        place(ctx, Box, Vector3 { 0.f, 2.f, -1.25f }, upright,
              Diag3x3 { 24.f, 30.f, 0.5f }, kPlainOverride);
        sun(ctx, sunDir());
        break;
    case 10:
        // tops at exactly the height of viewer 0 (none of them under its very
        // centre: the only ray of a one-pixel image runs past them)
        for (int32_t i = 0; i < 3; i++) {
            place(ctx, Box, Vector3 { -4.f + 2.75f * (float)i, 5.f + (float)i, 0.75f },
                  upright, Diag3x3 { 2.f, 2.f, 1.5f },
                  i == 1 ? kColor : kDefault, 0x4060E0u);
        }
        place(ctx, Box, Vector3 { 0.6f, 11.f, 1.9f }, upright,
              Diag3x3 { 10.f, 1.f, 5.f }, kPlainOverride);
        sun(ctx, sunDir());
        break;
    case 11:
        everyMesh(ctx);
        break;
    case 12: case 13:
        place(ctx, Box, Vector3 { 0.f, 8.f, 1.5f }, upright,
              Diag3x3 { 9.f, 1.f, 6.f });
        place(ctx, Ellipsoid, Vector3 { 0.5f, 5.f, 0.5f }, tilted(),
              Diag3x3 { 1.5f, 2.5f, 1.5f });
        for (int32_t i = 0; i < 8; i++) {
            // kind 12: each of the eight adds about an eighth to the wall's
            // front; kind 13: the eight come from behind the wall
            const float towards = 0.09f + 0.01f * (float)i;
            sun(ctx, Vector3 { 0.1f * (float)(i - 4), kind == 12 ? towards : -towards,
                               -0.2f - 0.05f * (float)(i % 3) });
        }
        if (kind == 13) {
            sun(ctx, Vector3 { 0.2f, 0.9f, -0.3f });
        }
        break;
    case 14:
        place(ctx, Box, Vector3 { 0.f, 9.2f, 2.f }, upright,
              Diag3x3 { 14.f, 1.f, 8.f }, kPlainOverride);
        place(ctx, Box, Vector3 { 0.f, 5.f, -1.25f }, upright,
              Diag3x3 { 14.f, 9.f, 0.5f });
        // between the third lamp and the wall
        place(ctx, Box, Vector3 { 3.f, 5.5f, 2.5f }, quat(1.f, 0.2f, 0.1f, 0.3f),
              Diag3x3 { 1.2f, 1.2f, 1.2f }, kColor, 0xE0A030u);
        place(ctx, Ellipsoid, Vector3 { -2.5f, 6.5f, 0.f }, tilted(),
              Diag3x3 { 1.2f, 2.f, 1.4f });
        // a cone whose edge crosses the wall
        light(ctx, false, Vector3 { -1.f, 2.f, 5.f }, Vector3 { 0.f, 0.86f, -0.5f },
              0.3f, false);
        // no cone: lights everything it faces, at a grazing angle
        light(ctx, false, Vector3 { -9.f, 7.5f, 2.f }, Vector3 { 1.f, 0.f, 0.f },
              -1.f, false);
        light(ctx, false, Vector3 { 4.f, 1.f, 4.f }, Vector3 { -0.2f, 0.9f, -0.3f },
              0.6f, true);
        break;
    default:
        // kind 15: spread over viewer 1's frustum, six columns by five rows
        for (int32_t i = 0; i < 30; i++) {
            const Vector3 pos { -3.6f + 1.55f * (float)(i % 6) + 0.1f * (float)(i / 6),
                                6.5f + 0.3f * (float)(i % 4),
                                -1.5f + 1.6f * (float)(i / 6) };
            const int32_t object = i % 5;
            if (object == Box) {
                place(ctx, Box, pos, quat(1.f, 0.f, 0.1f, 0.05f * (float)(i % 3)),
                      Diag3x3 { 1.2f, 0.8f, 1.1f }, i % 2 == 0 ? kColor : kDefault,
                      (uint32_t)(i * 524287));
            } else {
                place(ctx, object, pos, quat(1.f, 0.3f, 0.1f * (float)(i % 7) + 0.05f, 0.2f),
                      Diag3x3 { 0.9f, 1.3f, object == Ellipsoid ? 0.6f : 1.6f },
                      i == 13 ? kTexturedOverride : kDefault);
            }
        }
        sun(ctx, sunDir());
        break;
    }

    // viewer 0: axis-aligned, 90 degrees; viewer 1: generally rotated (turned
    // left, pitched down, rolled), 60 degrees, camera above the entity
    Entity v0 = ctx.makeEntity<Viewer>();
    ctx.get<Position>(v0) = Vector3 { 0.f, 0.f, 1.5f };
    ctx.get<Rotation>(v0) = upright;
    RenderingSystem::attachEntityToView(ctx, v0, 90.f, 0.125f, Vector3::zero());

    Entity v1 = ctx.makeEntity<Viewer>();
    ctx.get<Position>(v1) = Vector3 { 1.f, -1.5f, 1.75f };
    ctx.get<Rotation>(v1) = quat(1.f, -0.05f, 0.04f, 0.05f);
    RenderingSystem::attachEntityToView(ctx, v1, 60.f, 0.125f,
                                        Vector3 { 0.f, 0.f, 0.25f });
}

#ifdef MADRONA_GPU_MODE
MADRONA_BUILD_MWGPU_ENTRY(Engine, Sim, Sim::Config, Sim::WorldInit);
#endif

}
