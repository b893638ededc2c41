// TEST INFRASTRUCTURE.  One world's solver phases through the overlay's SCALAR
// XPBD routines (phys_impl/xpbd.hpp: integrateBody, handleContact<StoreT>,
// handleJointConstraint<StoreT>, deriveVelocity, solveVelocitiesForContact<
// StoreT>) over an array-backed body store, constraints in index order -- the
// math physicsStepKernel runs.  Shared by the host shim (phys_host_shim.cpp) and
// mode 0 of the device shim (phys_device_shim.hip).  The flat layout is the one
// documented in oracle/ref_shims/xpbd_ref_shim.cpp.
#pragma once

#include <madrona/physics.hpp>
#include <madrona/phys_impl/xpbd.hpp>

namespace solver_world {

using namespace madrona;
using namespace madrona::phys;
using madrona::math::Vector3;
using madrona::math::Vector4;
using madrona::math::Quat;

constexpr int32_t kMaxBodies = 64;
constexpr int32_t kBodyStride = 48;
constexpr int32_t kBodyState = 33;
constexpr int32_t kContactStride = 20;
constexpr int32_t kJointStride = 20;

struct Body {
    Vector3 x;
    Quat q;
    Velocity vel;
    xpbd::SubstepPrevState prev;
    xpbd::PreSolvePositional pre;
    xpbd::PreSolveVelocity preVel;
    RigidBodyMetadata metadata;
    ResponseType type;
    Vector3 extForce;
    Vector3 extTorque;
};

MADRONA_HD inline Vector3 vec3(const float *p)
{
    return Vector3 { p[0], p[1], p[2] };
}

MADRONA_HD inline Quat quat(const float *p)
{
    return Quat { p[0], p[1], p[2], p[3] };
}

MADRONA_HD inline void put3(float *p, Vector3 v)
{
    p[0] = v.x; p[1] = v.y; p[2] = v.z;
}

MADRONA_HD inline void put4(float *p, Quat q)
{
    p[0] = q.w; p[1] = q.x; p[2] = q.y; p[3] = q.z;
}

MADRONA_HD inline Body loadBody(const float *b, int32_t type)
{
    Body body {};
    body.x = vec3(b + 0);
    body.q = quat(b + 3);
    body.vel = Velocity { vec3(b + 7), vec3(b + 10) };
    body.prev = xpbd::SubstepPrevState { vec3(b + 13), quat(b + 16) };
    body.pre = xpbd::PreSolvePositional { vec3(b + 20), quat(b + 23) };
    body.preVel = xpbd::PreSolveVelocity { vec3(b + 27), vec3(b + 30) };
    body.metadata.mass.invMass = b[33];
    body.metadata.mass.invInertiaTensor = vec3(b + 34);
    body.metadata.friction.muS = b[37];
    body.metadata.friction.muD = b[38];
    body.type = (ResponseType)type;
    body.extForce = vec3(b + 39);
    body.extTorque = vec3(b + 42);
    return body;
}

MADRONA_HD inline void storeBody(const Body &body, float *o)
{
    put3(o + 0, body.x);
    put4(o + 3, body.q);
    put3(o + 7, body.vel.linear);
    put3(o + 10, body.vel.angular);
    put3(o + 13, body.prev.prevPosition);
    put4(o + 16, body.prev.prevRotation);
    put3(o + 20, body.pre.x);
    put4(o + 23, body.pre.q);
    put3(o + 27, body.preVel.v);
    put3(o + 30, body.preVel.omega);
}

// what xpbd::handleContact & co. ask of a body store; Loc::row names the body
struct ArrayBodyStore {
    Body *bodies;

    MADRONA_HD inline Vector3 &position(Loc l) { return bodies[l.row].x; }
    MADRONA_HD inline Quat &rotation(Loc l) { return bodies[l.row].q; }
    MADRONA_HD inline Velocity &velocity(Loc l) { return bodies[l.row].vel; }

    MADRONA_HD inline xpbd::SubstepPrevState prevState(Loc l)
    {
        return bodies[l.row].prev;
    }

    MADRONA_HD inline xpbd::PreSolvePositional presolvePositional(Loc l)
    {
        return bodies[l.row].pre;
    }

    MADRONA_HD inline xpbd::PreSolveVelocity presolveVelocity(Loc l)
    {
        return bodies[l.row].preVel;
    }

    MADRONA_HD inline xpbd::BodyConstants constants(Loc l)
    {
        return xpbd::bodyConstants(bodies[l.row].metadata, bodies[l.row].type);
    }
};

MADRONA_HD inline bool loadContact(const float *c, const int32_t *ci,
                                   int32_t num_bodies, ContactConstraint *out)
{
    if (ci[0] < 0 || ci[0] >= num_bodies || ci[1] < 0 ||
            ci[1] >= num_bodies || ci[2] < 0 || ci[2] > 4) {
        return false;
    }
    out->ref = Loc { 1, ci[0] };
    out->alt = Loc { 1, ci[1] };
    out->numPoints = ci[2];
    out->normal = vec3(c);
    for (int32_t p = 0; p < 4; p++) {
        out->points[p] = Vector4 { c[3 + 4 * p], c[4 + 4 * p], c[5 + 4 * p],
                                   c[6 + 4 * p] };
    }
    return true;
}

// (e1 / e2 stay unset: the store-taking solve names the bodies by Loc)
MADRONA_HD inline bool loadJoint(const float *j, const int32_t *ji,
                                 int32_t num_bodies, JointConstraint *out)
{
    if (ji[0] < 0 || ji[0] > 1 || ji[1] < 0 || ji[1] >= num_bodies ||
            ji[2] < 0 || ji[2] >= num_bodies) {
        return false;
    }
    out->r1 = vec3(j + 0);
    out->r2 = vec3(j + 3);
    if (ji[0] == 0) {
        out->type = JointConstraint::Type::Fixed;
        out->fixed.attachRot1 = quat(j + 6);
        out->fixed.attachRot2 = quat(j + 10);
        out->fixed.separation = j[14];
    } else {
        out->type = JointConstraint::Type::Hinge;
        out->hinge.a1Local = vec3(j + 6);
        out->hinge.a2Local = vec3(j + 9);
        out->hinge.b1Local = Vector3::zero();
        out->hinge.b2Local = Vector3::zero();
    }
    return true;
}

// `work`: num_bodies Body records of workspace
MADRONA_HD inline int32_t solveWorldScalar(
    const float *bodies, const int32_t *body_types, int32_t num_bodies,
    const float *contacts, const int32_t *contact_ints, int32_t num_contacts,
    const float *joints, const int32_t *joint_ints, int32_t num_joints,
    const float *sys, uint32_t phase_mask, float *bodies_out, float *lambdas,
    Body *work)
{
    if (num_bodies < 0 || num_bodies > kMaxBodies) return -1;

    const float h = sys[0];
    const Vector3 gravity = vec3(sys + 1);
    const float restitution_threshold = sys[4];

    for (int32_t i = 0; i < num_bodies; i++) {
        work[i] = loadBody(bodies + (size_t)i * kBodyStride, body_types[i]);
    }
    ArrayBodyStore store { work };

    if (phase_mask & 1u) {
        // physics.inl substepRigidBodies around xpbd::integrateBody
        for (int32_t i = 0; i < num_bodies; i++) {
            Body &b = work[i];
            b.prev.prevPosition = b.x;
            b.prev.prevRotation = b.q;
            if (b.type == ResponseType::Static) {
                b.pre.x = b.x;
                b.pre.q = b.q;
                b.preVel.v = Vector3::zero();
                b.preVel.omega = Vector3::zero();
                continue;
            }
            xpbd::SubstepResult next = xpbd::integrateBody(
                b.x, b.q, b.vel.linear, b.vel.angular,
                b.metadata.mass.invMass, b.metadata.mass.invInertiaTensor,
                b.extForce, b.extTorque, gravity, h,
                b.type == ResponseType::Dynamic);
            b.x = next.x;
            b.q = next.q;
            b.pre.x = next.x;
            b.pre.q = next.q;
            b.preVel.v = next.v;
            b.preVel.omega = next.omega;
        }
    }

    if (phase_mask & 2u) {
        for (int32_t i = 0; i < num_contacts; i++) {
            ContactConstraint contact;
            if (!loadContact(contacts + (size_t)i * kContactStride,
                             contact_ints + (size_t)i * 3, num_bodies,
                             &contact)) {
                return -2;
            }
            float lambda_n[4] { 0.f, 0.f, 0.f, 0.f };
            xpbd::handleContact(store, contact, lambda_n);
            lambdas[i] = lambda_n[0];
        }
    }

    if (phase_mask & 4u) {
        for (int32_t i = 0; i < num_joints; i++) {
            const int32_t *ji = joint_ints + (size_t)i * 3;
            JointConstraint joint;
            if (!loadJoint(joints + (size_t)i * kJointStride, ji, num_bodies,
                           &joint)) {
                return -3;
            }
            xpbd::handleJointConstraint(store, Loc { 1, ji[1] },
                                        Loc { 1, ji[2] }, joint);
        }
    }

    if (phase_mask & 8u) {
        for (int32_t i = 0; i < num_bodies; i++) {
            work[i].vel = xpbd::deriveVelocity(work[i].x, work[i].q,
                                               work[i].prev, h);
        }
    }

    if (phase_mask & 16u) {
        for (int32_t i = 0; i < num_contacts; i++) {
            ContactConstraint contact;
            if (!loadContact(contacts + (size_t)i * kContactStride,
                             contact_ints + (size_t)i * 3, num_bodies,
                             &contact)) {
                return -2;
            }
            float lambda_n[4] { lambdas[i], 0.f, 0.f, 0.f };
            xpbd::solveVelocitiesForContact(store, contact, lambda_n, h,
                                            restitution_threshold);
        }
    }

    for (int32_t i = 0; i < num_bodies; i++) {
        storeBody(work[i], bodies_out + (size_t)i * kBodyState);
    }
    return 0;
}

}
