// TEST INFRASTRUCTURE ONLY.  Exposes the reference's XPBD solver phases behind a
// C ABI so tests can compare madrona_amd's solver math with the reference's own
// code over a flat description of one world.  The solver routines are
// file-static in the reference, so the translation unit is included where it
// lies (nothing is copied).
//
// The phases are the reference's own Context-taking routines: the shim builds a
// real reference StateManager (base + physics + XPBD types registered, one
// rigid-body archetype, one world), creates one entity per body, writes the
// flat description into the ECS columns and the singletons, and calls
// substepRigidBodies / handleContact / handleJointConstraint / setVelocities /
// solveVelocitiesForContact on them.  Nothing of the solver is restated here.
//
// Flat layout (shared with tests/shims: tests/solver_utils.py is the authority)
//   body   48 floats: pos3 rot4(wxyz) vlin3 vang3 | prevPos3 prevRot4 |
//                     preX3 preQ4 | preV3 preOmega3 || invMass invI3 muS muD
//                     extForce3 extTorque3 pad3.  The first 33 are the state
//                     written back.
//   body_types  ResponseType per body (0 Dynamic, 1 Kinematic, 2 Static)
//   contact 20 floats: normal3, 4 x (point3, depth), pad;  3 ints: ref alt n
//   joint   20 floats: r1(3) r2(3), then Fixed: attachRot1(4) attachRot2(4)
//                     separation | Hinge: a1Local(3) a2Local(3);
//                     3 ints: type (0 Fixed, 1 Hinge), body1, body2
//   sys     5 floats: h, gravity3, restitution threshold
//   lambdas in/out, one per contact: phase 2 overwrites, phase 5 reads
#include <madrona/physics.hpp>
#include <madrona/context.hpp>
#include <madrona/registry.hpp>
#include <madrona/components.hpp>

#include "../../../reference/src/core/worker_init.hpp"
#include "../../../reference/src/physics/physics_impl.hpp"

// the solver's routines are static / inline in this TU: pull it in
#include "../../../reference/src/physics/xpbd.cpp"

#include <cstring>

using namespace madrona;
using namespace madrona::phys;
using namespace madrona::math;

namespace {

constexpr int32_t kMaxBodies = 64;
constexpr int32_t kBodyStride = 48;
constexpr int32_t kBodyState = 33;
constexpr int32_t kContactStride = 20;
constexpr int32_t kJointStride = 20;

struct ShimBody : Archetype<RigidBody> {};

struct RefWorld {
    StateManager mgr;
    StateCache cache;
    void *exportPtrs[1];
    Context *ctx;
    Entity bodies[kMaxBodies];
    Loc locs[kMaxBodies];
    RigidBodyMetadata metadata[kMaxBodies];
    ObjectManager objMgr;

    RefWorld() : mgr(1), cache(), exportPtrs { nullptr }
    {
        ECSRegistry registry(&mgr, exportPtrs);
        base::registerTypes(registry);
        PhysicsSystem::registerTypes(registry, PhysicsSystem::Solver::XPBD);
        registry.registerArchetype<ShimBody>();

        ctx = new Context(nullptr, WorkerInit { &mgr, &cache, 0u });
        for (int32_t i = 0; i < kMaxBodies; i++) {
            bodies[i] = ctx->makeEntity<ShimBody>();
        }
        for (int32_t i = 0; i < kMaxBodies; i++) {
            locs[i] = ctx->loc(bodies[i]);
        }

        memset(&objMgr, 0, sizeof(objMgr));
        objMgr.metadata = metadata;
        ctx->singleton<ObjectData>().mgr = &objMgr;
    }
};

RefWorld &world()
{
    static RefWorld *w = new RefWorld();
    return *w;
}

inline Vector3 vec3(const float *p) { return Vector3 { p[0], p[1], p[2] }; }
inline Quat quat(const float *p) { return Quat { p[0], p[1], p[2], p[3] }; }
inline void put3(float *p, Vector3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
inline void put4(float *p, Quat q)
{
    p[0] = q.w; p[1] = q.x; p[2] = q.y; p[3] = q.z;
}

}

extern "C" {

#define API __attribute__((visibility("default")))

API int32_t ref_solve_world(const float *bodies, const int32_t *body_types,
                            int32_t num_bodies,
                            const float *contacts, const int32_t *contact_ints,
                            int32_t num_contacts,
                            const float *joints, const int32_t *joint_ints,
                            int32_t num_joints,
                            const float *sys, uint32_t phase_mask,
                            float *bodies_out, float *lambdas)
{
    using namespace xpbd;

    if (num_bodies < 0 || num_bodies > kMaxBodies) return -1;

    RefWorld &w = world();
    Context &ctx = *w.ctx;

    PhysicsSystemState &physics_sys = ctx.singleton<PhysicsSystemState>();
    memset(&physics_sys, 0, sizeof(physics_sys));
    physics_sys.h = sys[0];
    physics_sys.deltaT = sys[0];
    physics_sys.g = vec3(sys + 1);
    physics_sys.gMagnitude = physics_sys.g.length();
    physics_sys.restitutionThreshold = sys[4];

    for (int32_t i = 0; i < num_bodies; i++) {
        const float *b = bodies + (size_t)i * kBodyStride;
        Loc l = w.locs[i];
        ctx.getDirect<base::Position>(RGDCols::Position, l) = vec3(b + 0);
        ctx.getDirect<base::Rotation>(RGDCols::Rotation, l) = quat(b + 3);
        ctx.getDirect<base::Scale>(RGDCols::Scale, l) = Diag3x3 { 1, 1, 1 };
        ctx.getDirect<base::ObjectID>(RGDCols::ObjectID, l) =
            base::ObjectID { i };
        ctx.getDirect<ResponseType>(RGDCols::ResponseType, l) =
            (ResponseType)body_types[i];
        ctx.getDirect<Velocity>(RGDCols::Velocity, l) =
            Velocity { vec3(b + 7), vec3(b + 10) };
        ctx.getDirect<ExternalForce>(RGDCols::ExternalForce, l) = vec3(b + 39);
        ctx.getDirect<ExternalTorque>(RGDCols::ExternalTorque, l) =
            vec3(b + 42);
        ctx.getDirect<SubstepPrevState>(XPBDCols::SubstepPrevState, l) =
            SubstepPrevState { vec3(b + 13), quat(b + 16) };
        ctx.getDirect<PreSolvePositional>(XPBDCols::PreSolvePositional, l) =
            PreSolvePositional { vec3(b + 20), quat(b + 23) };
        ctx.getDirect<PreSolveVelocity>(XPBDCols::PreSolveVelocity, l) =
            PreSolveVelocity { vec3(b + 27), vec3(b + 30) };

        RigidBodyMetadata &m = w.metadata[i];
        memset(&m, 0, sizeof(m));
        m.mass.invMass = b[33];
        m.mass.invInertiaTensor = vec3(b + 34);
        m.mass.toInteriaFrame = Quat { 1, 0, 0, 0 };
        m.friction.muS = b[37];
        m.friction.muD = b[38];
    }

    auto contactAt = [&](int32_t i, ContactConstraint *out) {
        const float *c = contacts + (size_t)i * kContactStride;
        const int32_t *ci = contact_ints + (size_t)i * 3;
        if (ci[0] < 0 || ci[0] >= num_bodies || ci[1] < 0 ||
                ci[1] >= num_bodies || ci[2] < 0 || ci[2] > 4) {
            return false;
        }
        out->ref = w.locs[ci[0]];
        out->alt = w.locs[ci[1]];
        out->numPoints = ci[2];
        out->normal = vec3(c);
        for (int32_t p = 0; p < 4; p++) {
            out->points[p] = Vector4 { c[3 + 4 * p], c[4 + 4 * p],
                                       c[5 + 4 * p], c[6 + 4 * p] };
        }
        return true;
    };

    if (phase_mask & 1u) {
        for (int32_t i = 0; i < num_bodies; i++) {
            Loc l = w.locs[i];
            substepRigidBodies(ctx,
                ctx.getDirect<base::Position>(RGDCols::Position, l),
                ctx.getDirect<base::Rotation>(RGDCols::Rotation, l),
                ctx.getDirect<Velocity>(RGDCols::Velocity, l),
                ctx.getDirect<base::ObjectID>(RGDCols::ObjectID, l),
                ctx.getDirect<ResponseType>(RGDCols::ResponseType, l),
                ctx.getDirect<ExternalForce>(RGDCols::ExternalForce, l),
                ctx.getDirect<ExternalTorque>(RGDCols::ExternalTorque, l),
                ctx.getDirect<SubstepPrevState>(
                    XPBDCols::SubstepPrevState, l),
                ctx.getDirect<PreSolvePositional>(
                    XPBDCols::PreSolvePositional, l),
                ctx.getDirect<PreSolveVelocity>(
                    XPBDCols::PreSolveVelocity, l));
        }
    }

    if (phase_mask & 2u) {
        for (int32_t i = 0; i < num_contacts; i++) {
            ContactConstraint contact;
            if (!contactAt(i, &contact)) return -2;
            // as solvePositions does before each handleContact
            float lambda_n[4] { 0.f, 0.f, 0.f, 0.f };
            handleContact(ctx, w.objMgr, contact, lambda_n);
            lambdas[i] = lambda_n[0];
        }
    }

    if (phase_mask & 4u) {
        for (int32_t i = 0; i < num_joints; i++) {
            const float *j = joints + (size_t)i * kJointStride;
            const int32_t *ji = joint_ints + (size_t)i * 3;
            if (ji[1] < 0 || ji[1] >= num_bodies || ji[2] < 0 ||
                    ji[2] >= num_bodies || ji[0] < 0 || ji[0] > 1) {
                return -3;
            }
            JointConstraint joint;
            memset(&joint, 0, sizeof(joint));
            joint.e1 = w.bodies[ji[1]];
            joint.e2 = w.bodies[ji[2]];
            joint.r1 = vec3(j + 0);
            joint.r2 = vec3(j + 3);
            if (ji[0] == 0) {
                joint.type = JointConstraint::Type::Fixed;
                joint.fixed.attachRot1 = quat(j + 6);
                joint.fixed.attachRot2 = quat(j + 10);
                joint.fixed.separation = j[14];
            } else {
                joint.type = JointConstraint::Type::Hinge;
                joint.hinge.a1Local = vec3(j + 6);
                joint.hinge.a2Local = vec3(j + 9);
            }
            handleJointConstraint(ctx, joint);
        }
    }

    if (phase_mask & 8u) {
        for (int32_t i = 0; i < num_bodies; i++) {
            Loc l = w.locs[i];
            setVelocities(ctx,
                ctx.getDirect<base::Position>(RGDCols::Position, l),
                ctx.getDirect<base::Rotation>(RGDCols::Rotation, l),
                ctx.getDirect<SubstepPrevState>(
                    XPBDCols::SubstepPrevState, l),
                ctx.getDirect<Velocity>(RGDCols::Velocity, l));
        }
    }

    if (phase_mask & 16u) {
        for (int32_t i = 0; i < num_contacts; i++) {
            ContactConstraint contact;
            if (!contactAt(i, &contact)) return -2;
            float lambda_n[4] { lambdas[i], 0.f, 0.f, 0.f };
            solveVelocitiesForContact(ctx, w.objMgr, contact, lambda_n,
                physics_sys.h, physics_sys.restitutionThreshold);
        }
    }

    for (int32_t i = 0; i < num_bodies; i++) {
        float *o = bodies_out + (size_t)i * kBodyState;
        Loc l = w.locs[i];
        put3(o + 0, ctx.getDirect<base::Position>(RGDCols::Position, l));
        put4(o + 3, ctx.getDirect<base::Rotation>(RGDCols::Rotation, l));
        Velocity v = ctx.getDirect<Velocity>(RGDCols::Velocity, l);
        put3(o + 7, v.linear);
        put3(o + 10, v.angular);
        SubstepPrevState prev = ctx.getDirect<SubstepPrevState>(
            XPBDCols::SubstepPrevState, l);
        put3(o + 13, prev.prevPosition);
        put4(o + 16, prev.prevRotation);
        PreSolvePositional pre = ctx.getDirect<PreSolvePositional>(
            XPBDCols::PreSolvePositional, l);
        put3(o + 20, pre.x);
        put4(o + 23, pre.q);
        PreSolveVelocity pre_vel = ctx.getDirect<PreSolveVelocity>(
            XPBDCols::PreSolveVelocity, l);
        put3(o + 27, pre_vel.v);
        put3(o + 30, pre_vel.omega);
    }

    return 0;
}

}
