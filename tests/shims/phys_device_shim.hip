// TEST INFRASTRUCTURE.  madrona_amd's narrowphase code paths run ON THE DEVICE,
// pair by pair, behind the C ABI of the host shim (phys_host_shim.cpp), so the
// GPU tests can diff them function by function against the reference's
// narrowphase (oracle/_ref/libphys_ref.so):
//   mode 0  collidePairStored   one lane per pair, hulls in private scratch
//                               (the > 128-body kernel, and the fallback of
//                               the LDS kernel for big faces)
//   mode 1  collidePairLane     one lane per pair, LazyHull + an LDS row (the
//                               LDS kernel's plane / sphere path)
//   mode 2  hullHullWave        one wavefront per pair (the LDS kernel's
//                               cooperative hull-hull SAT)
//   mode 3  hullHullWave<32>    two pairs per wavefront, 32 lanes each
//   mode 4  hullHullWave<16>    four pairs per wavefront, 16 lanes each (what
//                               the two-worlds-per-wavefront kernel runs)
// and the XPBD solve, world by world, behind the layout of
// oracle/ref_shims/xpbd_ref_shim.cpp (dev_solve_worlds):
//   mode 0  the scalar routines of phys_impl/xpbd.hpp, one lane per world
//           (solver_world.hpp: what the host shim runs, compiled for the device)
//   mode 1  solveSubstepConstraints<64, 64>   the LDS step kernel's own solve
//   mode 2  solveSubstepConstraints<32, 32>   (phys_impl/step_solve.inl) over a
//   mode 3  solveSubstepConstraints<128, 64>  real WorldBlock and LdsBodyStore;
//           <32, 32>: two worlds per wavefront, neighbours share one
// plus the level rule and the bit selection its loops stand on
// (dev_constraint_levels, dev_nth_set_bit).
#include <madrona/mwhip/user_prelude.hpp>
// (the physics headers are written like simulator sources: unannotated
// definitions, made host + device by the wrapper's pragma -- madrona_amd/Makefile)
#pragma clang force_cuda_host_device begin
#include <madrona/physics.hpp>
#include <madrona/physics_assets.hpp>
#include <madrona/physics_loader.hpp>
#pragma clang force_cuda_host_device end

#include "solver_world.hpp"

#include <vector>

using namespace madrona;
using namespace madrona::phys;
using namespace madrona::phys::narrowphase;

namespace {

struct PairIn {
    float a[10];    // pos xyz, rot wxyz, scale xyz
    float b[10];
};

__device__ inline PrimitiveTransform loadTxfm(const float *t)
{
    return PrimitiveTransform {
        { t[0], t[1], t[2] }, { t[3], t[4], t[5], t[6] }, { t[7], t[8], t[9] } };
}

__device__ inline void storeContact(bool has, const ContactConstraint &c,
                                    int32_t kind, float *out)
{
    // layout of phys_ref_shim.cpp: has, ref-is-a, numPoints, normal, points
    out[0] = has ? 1.f : 0.f;
    out[1] = has && kind == 0 && c.ref.archetype == 1 ? 1.f : 0.f;
    out[2] = has ? (float)c.numPoints : 0.f;
    out[3] = has ? c.normal.x : 0.f;
    out[4] = has ? c.normal.y : 0.f;
    out[5] = has ? c.normal.z : 0.f;
    for (int i = 0; i < 4; i++) {
        out[6 + 4 * i + 0] = has ? c.points[i].x : 0.f;
        out[6 + 4 * i + 1] = has ? c.points[i].y : 0.f;
        out[6 + 4 * i + 2] = has ? c.points[i].z : 0.f;
        out[6 + 4 * i + 3] = has ? c.points[i].w : 0.f;
    }
}

__global__ void __launch_bounds__(64)
collideKernel(const ObjectManager *obj_mgr, const PairIn *pairs,
              uint32_t num_pairs, int32_t kind, int32_t mode, float *out,
              int32_t *flags)
{
    __shared__ kernels::WaveScratch scratch;
    __shared__ kernels::HullScratch group_scratch[4];

    const uint32_t lane = threadIdx.x;
    // lanes per pair and pairs per wavefront of the cooperative modes
    const uint32_t group_lanes = mode == 3 ? 32u : (mode == 4 ? 16u : 64u);
    const uint32_t group = lane / group_lanes;
    const uint32_t p = mode == 2 ? blockIdx.x :
        (mode >= 3 ? blockIdx.x * (64u / group_lanes) + group :
                     blockIdx.x * 64 + lane);
    const bool active = p < num_pairs;

    PairSetup pair {};
    if (active) {
        pair.aLoc = Loc { 1, 0 };
        pair.bLoc = Loc { 2, 0 };
        pair.aPrim = &obj_mgr->collisionPrimitives[kind == 2 ? 2 : 0];
        pair.bPrim = &obj_mgr->collisionPrimitives[kind == 1 ? 1 : 0];
        pair.a = loadTxfm(pairs[p].a);
        pair.b = loadTxfm(pairs[p].b);
        pair.test = kind == 1 ? NarrowphaseTest::HullPlane :
            kind == 2 ? NarrowphaseTest::SphereHull :
                        NarrowphaseTest::HullHull;
        pair.aabbOverlap = true;
    }

    ContactConstraint contact {};
    bool has = false;
    bool too_big = false;
    bool unsupported = false;

    if (mode == 0) {
        constexpr int32_t max_elems = MADRONA_PHYS_MAX_HULL_ELEMS;
        geo::Plane tmp_faces[max_elems];
        math::Vector3 tmp_vertices[max_elems];
        if (active) {
            has = collidePairStored(pair, tmp_vertices, tmp_faces, max_elems,
                                    &contact, &unsupported);
        }
    } else if (mode == 1) {
        // lanes take turns on the LDS rows, as in the step kernel
        for (uint32_t first = 0; first < 64; first += kernels::lanePolyRows) {
            if (active && lane >= first &&
                    lane < first + kernels::lanePolyRows) {
                has = kernels::collidePairLane(pair,
                    scratch.lanePoly + (lane - first) * kernels::lanePolyDwords,
                    &contact, &too_big, &unsupported);
            }
        }
    } else if (mode == 2) {
        if (active) {   // wave-uniform
            has = kernels::hullHullWave(lane, pair, &scratch.hull, &contact,
                                        &too_big);
        }
    } else if (mode == 3) {
        if (active) {   // uniform per 32-lane group
            has = kernels::hullHullWave<32>(lane % 32u, pair,
                &group_scratch[group], &contact, &too_big);
        }
    } else {
        if (active) {   // uniform per 16-lane group
            has = kernels::hullHullWave<16>(lane % 16u, pair,
                &group_scratch[group], &contact, &too_big);
        }
    }

    if (active && (mode < 2 || lane % group_lanes == 0)) {
        storeContact(has, contact, kind, out + (size_t)p * 28);
        flags[p] = (too_big ? 1 : 0) | (unsupported ? 2 : 0);
    }
}

// The reference's own known-answer tests for code on this path, evaluated by
// the overlay's headers ON THE DEVICE: tests/math.cpp:23-48 (quaternions) and
// tests/gjk.cpp:19-48 (simplex sub-solvers of the sphere-hull GJK).
__global__ void katKernel(float *out)
{
    using math::Quat;
    using math::Vector3;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;

    Quat q1 = Quat::angleAxis(0, { 0, 1, 0 });
    Quat q2 = Quat::angleAxis(math::toRadians(45), { 0, 1, 0 });
    Quat q3 = Quat::angleAxis(math::toRadians(45), { 1, 0, 0 });
    Quat m1 = q2 * q3;
    const Quat qs[4] = { q1, q2, q3, m1 };
    for (int i = 0; i < 4; i++) {
        out[4 * i + 0] = qs[i].w;
        out[4 * i + 1] = qs[i].x;
        out[4 * i + 2] = qs[i].y;
        out[4 * i + 3] = qs[i].z;
    }

    {
        Vector3 Y[4] {
            { 0.814353108f, 0.195752025f, -0.698764443f },
            { -0.784147143f, 0.126484752f, 0.701235533f },
            { -0.784147143f, 0.126484752f, -0.698764443f },
            { -0.784147143f, 0.126484752f, 0.701235533f },
        };
        gjk::SimplexSolve s3 = gjk::solveTriangle(Y[0], Y[1], Y[2]);
        gjk::SimplexSolve s4 = gjk::solveTetrahedron(Y[0], Y[1], Y[2], Y[3]);
        out[16] = s3.vLen2;
        out[17] = s4.vLen2;
    }
    {
        Vector3 Y[4] {
            { 0.793287277f, 2.86326122f, -0.700307727f },
            { -0.794485092f, -0.542466521f, 0.699692249f },
            { 0.80550468f, -0.536717057f, -0.700307727f },
            { -0.794485092f, -0.542466521f, -0.700307727f },
        };
        gjk::SimplexSolve s = gjk::solveTetrahedron(Y[0], Y[1], Y[2], Y[3]);
        out[18] = s.v.x;
        out[19] = s.v.y;
        out[20] = s.v.z;
        out[21] = s.vLen2;
    }
}

// ---------------------------------------------------------------------------
// the XPBD solve
// ---------------------------------------------------------------------------
struct SolveArgs {
    const float *bodies;
    const int32_t *bodyTypes;
    const int32_t *bodyOff;
    const float *contacts;
    const int32_t *contactInts;
    const int32_t *contactOff;
    const float *joints;
    const int32_t *jointInts;
    const int32_t *jointOff;
    const float *sys;
    uint32_t phaseMask;
    int32_t numWorlds;
    float *bodiesOut;
    float *lambdas;
    int32_t *status;
    solver_world::Body *work;       // mode 0: a record per body
    JointConstraint *jointRows;     // modes 1-3: the "sorted joint table"
};

__global__ void __launch_bounds__(64)
solveScalarKernel(SolveArgs a)
{
    const int32_t world = (int32_t)(blockIdx.x * 64 + threadIdx.x);
    if (world >= a.numWorlds) return;

    const int32_t b0 = a.bodyOff[world];
    const int32_t c0 = a.contactOff[world];
    const int32_t j0 = a.jointOff[world];
    a.status[world] = solver_world::solveWorldScalar(
        a.bodies + (size_t)b0 * solver_world::kBodyStride, a.bodyTypes + b0,
        a.bodyOff[world + 1] - b0,
        a.contacts + (size_t)c0 * solver_world::kContactStride,
        a.contactInts + (size_t)c0 * 3, a.contactOff[world + 1] - c0,
        a.joints + (size_t)j0 * solver_world::kJointStride,
        a.jointInts + (size_t)j0 * 3, a.jointOff[world + 1] - j0,
        a.sys + (size_t)world * 5, a.phaseMask,
        a.bodiesOut + (size_t)b0 * solver_world::kBodyState, a.lambdas + c0,
        a.work + b0);
}

// Fills the block as the step kernel leaves it in front of its solve (poses and
// the substep's records, pre-solve velocities, constants, keys and slots,
// packed contacts, joints, system state); one lane of the world's group does it.
// solverKey / solverSlot: the rule of physicsStepLdsKernel's load -- a Static
// body that the solver's writes leave as it is (staticBodyIsInert) gets key 0
// and no slot, every other body key k + 1 and the next slot.
// Returns 0, or < 0 when the block cannot hold the world.
template <int MAXB, int LPW>
__device__ inline int32_t fillBlock(kernels::WorldBlock<MAXB, LPW> *w,
                                    const SolveArgs &a, int32_t world)
{
    using Block = kernels::WorldBlock<MAXB, LPW>;
    using namespace solver_world;

    const int32_t b0 = a.bodyOff[world];
    const int32_t nb = a.bodyOff[world + 1] - b0;
    const int32_t c0 = a.contactOff[world];
    const int32_t nc = a.contactOff[world + 1] - c0;
    const int32_t j0 = a.jointOff[world];
    const int32_t nj = a.jointOff[world + 1] - j0;
    if (nb < 0 || nb > MAXB || nb > kMaxBodies) return -1;
    if (nc < 0 || nc > Block::maxContacts) return -5;
    if (nj < 0 || nj > Block::maxJointBodies) return -6;

    uint32_t solver_bodies = 0;
    for (int32_t k = 0; k < nb; k++) {
        const Body body = loadBody(a.bodies + (size_t)(b0 + k) * kBodyStride,
                                   a.bodyTypes[b0 + k]);
        const bool solved = !(body.type == ResponseType::Static &&
                              kernels::staticBodyIsInert(body.x, body.q));
        if (solved && solver_bodies >= (uint32_t)Block::maxSolverBodies) {
            return -4;
        }
        w->poses[k] = typename Block::Pose { body.x, body.q };
        w->scale[k] = math::Diag3x3 { 1, 1, 1 };
        w->vel[k] = body.vel;
        w->constants[k] = xpbd::bodyConstants(body.metadata, body.type);
        w->resp[k] = (uint8_t)body.type;
        w->solverKey[k] = solved ? (uint8_t)(k + 1) : (uint8_t)0;
        w->solverSlot[k] = solved ? (uint8_t)solver_bodies :
                                    (uint8_t)Block::noSlot;
        if (solved) {
            w->poses[Block::prevBase + solver_bodies] = typename Block::Pose {
                body.prev.prevPosition, body.prev.prevRotation };
            w->poses[Block::prePosBase + solver_bodies] =
                typename Block::Pose { body.pre.x, body.pre.q };
            w->preVel[solver_bodies] = body.preVel;
            solver_bodies++;
        }
    }

    for (int32_t i = 0; i < nc; i++) {
        ContactConstraint c;
        if (!loadContact(a.contacts + (size_t)(c0 + i) * kContactStride,
                         a.contactInts + (size_t)(c0 + i) * 3, nb, &c)) {
            return -2;
        }
        w->contacts()[i] = kernels::PackedContact::pack(c);
        w->lambdas[i] = a.lambdas[c0 + i];
    }

    for (int32_t j = 0; j < nj; j++) {
        const int32_t *ji = a.jointInts + (size_t)(j0 + j) * 3;
        JointConstraint joint {};
        if (!loadJoint(a.joints + (size_t)(j0 + j) * kJointStride, ji, nb,
                       &joint)) {
            return -3;
        }
        // every row in the table; the first maxJoints of them in the block too
        a.jointRows[j0 + j] = joint;
        if (j < Block::maxJoints) {
            w->joints[j] = joint;
        }
        w->jointBodies[j][0] = (uint8_t)ji[1];
        w->jointBodies[j][1] = (uint8_t)ji[2];
    }

    const float *sys = a.sys + (size_t)world * 5;
    w->sys = PhysicsSystemState {};
    w->sys.deltaT = sys[0];
    w->sys.h = sys[0];
    w->sys.g = vec3(sys + 1);
    w->sys.restitutionThreshold = sys[4];
    return 0;
}

template <int MAXB, int LPW>
__global__ void __launch_bounds__(64)
solveBlockKernel(SolveArgs a)
{
    using Block = kernels::WorldBlock<MAXB, LPW>;
    constexpr int worlds_per_wave = 64 / LPW;

    __shared__ Block blocks[worlds_per_wave];
    __shared__ int32_t fill_status[worlds_per_wave];

    const uint32_t lane = kernels::wave::laneID() & (uint32_t)(LPW - 1);
    const int32_t group = (int32_t)(kernels::wave::laneID() / (uint32_t)LPW);
    const int32_t world = (int32_t)blockIdx.x * worlds_per_wave + group;
    Block *w = &blocks[group];
    kernels::LdsBodyStore<MAXB, LPW> store { w };

    // (per group from here on, as in the step kernel: the two halves of a
    // wavefront diverge where their worlds differ)
    if (world < a.numWorlds) {
        if (lane == 0) {
            fill_status[group] = fillBlock<MAXB, LPW>(w, a, world);
        }
        kernels::wave::phaseFence();
        const int32_t status = fill_status[group];

        if (status == 0) {
            const int32_t b0 = a.bodyOff[world];
            const int32_t nb = a.bodyOff[world + 1] - b0;
            const int32_t c0 = a.contactOff[world];
            const int32_t nc = a.contactOff[world + 1] - c0;
            const int32_t j0 = a.jointOff[world];
            const int32_t nj = a.jointOff[world + 1] - j0;

            kernels::solveSubstepConstraints<MAXB, LPW>(
                lane, w, store, nb, (uint32_t)nc, nj, a.jointRows + j0,
                [](int) {});
            kernels::wave::phaseFence();

            // what the step kernel's epilogue stores of a body
            for (int32_t k = (int32_t)lane; k < nb; k += LPW) {
                solver_world::Body body {};
                body.x = w->poses[k].x;
                body.q = w->poses[k].q;
                body.vel = w->vel[k];
                body.prev = store.prevState(Loc { 0, k });
                body.pre = store.presolvePositional(Loc { 0, k });
                body.preVel = store.presolveVelocity(Loc { 0, k });
                solver_world::storeBody(body, a.bodiesOut +
                    (size_t)(b0 + k) * solver_world::kBodyState);
            }
            for (int32_t i = (int32_t)lane; i < nc; i += LPW) {
                a.lambdas[c0 + i] = w->lambdas[i];
            }
        }
        if (lane == 0) {
            a.status[world] = status;
        }
    }
}

// levels of `cases` windows of up to LPW constraints, a window per group of LPW
// lanes (keys: cases x LPW, zero beyond counts[case])
template <int LPW>
__global__ void __launch_bounds__(64)
levelsKernel(const uint32_t *keys_a, const uint32_t *keys_b,
             const uint32_t *counts, uint32_t cases, uint32_t *levels)
{
    const uint32_t lane = kernels::wave::laneID() & (uint32_t)(LPW - 1);
    const uint32_t group = kernels::wave::laneID() / (uint32_t)LPW;
    const uint32_t c = blockIdx.x * (64u / LPW) + group;
    if (c < cases) {
        const uint32_t n = counts[c];
        levels[(size_t)c * LPW + lane] = kernels::constraintLevels<LPW>(
            lane, n, keys_a[(size_t)c * LPW + lane],
            keys_b[(size_t)c * LPW + lane]);
    }
}

template <int LPW>
__global__ void __launch_bounds__(64)
nthSetBitKernel(const uint64_t *masks, uint32_t cases, uint32_t *out)
{
    const uint32_t c = blockIdx.x;
    const uint32_t n = threadIdx.x;
    if (c < cases) {
        const uint64_t mask = masks[c];
        out[(size_t)c * 64 + n] =
            n < (uint32_t)__builtin_popcountll(mask) ?
                kernels::wave::nthSetBit<LPW>(mask, n) : 0xFFFFFFFFu;
    }
}

// device buffers of one export: freed together, a failed allocation shows
struct DeviceBuffers {
    std::vector<void *> ptrs;
    bool failed = false;

    template <typename T>
    T *alloc(size_t count, const T *src = nullptr)
    {
        void *p = nullptr;
        if (hipMalloc(&p, sizeof(T) * (count == 0 ? 1 : count)) != hipSuccess) {
            failed = true;
            return nullptr;
        }
        ptrs.push_back(p);
        if (src != nullptr && count != 0 &&
                hipMemcpy(p, src, sizeof(T) * count,
                          hipMemcpyHostToDevice) != hipSuccess) {
            failed = true;
        }
        return (T *)p;
    }

    ~DeviceBuffers()
    {
        for (void *p : ptrs) {
            (void)hipFree(p);
        }
    }
};

}

extern "C" {

#define API __attribute__((visibility("default")))

// out[22]: q1, q2, q3, q2*q3 (w x y z each), |v|^2 of the 3- and 4-simplex
// solves with a duplicated point, v and |v|^2 of the simplex around the origin
API int32_t dev_reference_kats(float *out)
{
    float *d_out = nullptr;
    if (hipMalloc(&d_out, sizeof(float) * 22) != hipSuccess) return -2;
    hipLaunchKernelGGL(katKernel, dim3(1), dim3(64), 0, 0, d_out);
    int32_t rc = hipDeviceSynchronize() == hipSuccess ? 0 : -3;
    (void)hipMemcpy(out, d_out, sizeof(float) * 22, hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    return rc;
}

// kind: 0 hull-hull, 1 hull-plane, 2 sphere (a) - hull (b); see modes above.
// out: num_pairs x 28 floats, flags: num_pairs (bit 0: face too big for the
// LDS scratch -- the caller falls back to mode 0 --, bit 1: unsupported).
API int32_t dev_collide_pairs(const float *verts, uint32_t num_verts,
                              const uint32_t *indices,
                              const uint32_t *face_counts, uint32_t num_faces,
                              const float *pairs, uint32_t num_pairs,
                              int32_t kind, int32_t mode, float *out,
                              int32_t *flags)
{
    imp::SourceMesh mesh {};
    mesh.positions = (math::Vector3 *)verts;
    mesh.indices = (uint32_t *)indices;
    mesh.faceCounts = (uint32_t *)face_counts;
    mesh.numVertices = num_verts;
    mesh.numFaces = num_faces;

    SourceCollisionPrimitive src_prims[3];
    src_prims[0].type = CollisionPrimitive::Type::Hull;
    src_prims[0].hullInput.hullIDX = 0;
    src_prims[1].type = CollisionPrimitive::Type::Plane;
    src_prims[2].type = CollisionPrimitive::Type::Sphere;
    src_prims[2].sphere.radius = 0.7f;
    SourceCollisionObject objs[3] = {
        { Span<const SourceCollisionPrimitive>(&src_prims[0], 1), 1.f, { 0.5f, 0.5f } },
        { Span<const SourceCollisionPrimitive>(&src_prims[1], 1), 0.f, { 0.5f, 0.5f } },
        { Span<const SourceCollisionPrimitive>(&src_prims[2], 1), 1.f, { 0.5f, 0.5f } },
    };

    StackAlloc tmp_alloc;
    RigidBodyAssets assets;
    CountT num_bytes;
    void *buf = RigidBodyAssets::processRigidBodyAssets(
        Span<const imp::SourceMesh>(&mesh, 1),
        Span<const SourceCollisionObject>(objs, 3),
        false, tmp_alloc, &assets, &num_bytes);
    if (buf == nullptr) return -1;

    PhysicsLoader loader(ExecMode::CUDA, 4, 0);
    loader.loadRigidBodies(assets);
    free(buf);

    PairIn *d_pairs = nullptr;
    float *d_out = nullptr;
    int32_t *d_flags = nullptr;
    if (hipMalloc(&d_pairs, sizeof(PairIn) * num_pairs) != hipSuccess ||
        hipMalloc(&d_out, sizeof(float) * 28 * num_pairs) != hipSuccess ||
        hipMalloc(&d_flags, sizeof(int32_t) * num_pairs) != hipSuccess) {
        return -2;
    }
    (void)hipMemcpy(d_pairs, pairs, sizeof(PairIn) * num_pairs,
                    hipMemcpyHostToDevice);

    const uint32_t blocks = mode == 2 ? num_pairs :
        mode == 3 ? (num_pairs + 1) / 2 :
        mode == 4 ? (num_pairs + 3) / 4 : (num_pairs + 63) / 64;
    hipLaunchKernelGGL(collideKernel, dim3(blocks), dim3(64), 0, 0,
                       &loader.getObjectManager(), d_pairs, num_pairs, kind,
                       mode, d_out, d_flags);
    int32_t rc = hipDeviceSynchronize() == hipSuccess ? 0 : -3;

    (void)hipMemcpy(out, d_out, sizeof(float) * 28 * num_pairs,
                    hipMemcpyDeviceToHost);
    (void)hipMemcpy(flags, d_flags, sizeof(int32_t) * num_pairs,
                    hipMemcpyDeviceToHost);
    (void)hipFree(d_pairs);
    (void)hipFree(d_out);
    (void)hipFree(d_flags);
    return rc;
}

// The solver phases in `phase_mask` (bit order of ref_solve_world) over
// num_worlds worlds laid end to end (body_off / contact_off / joint_off:
// num_worlds + 1 offsets each).  Modes 1-3 run the step kernel's solve, which is
// phases 2-5 together: phase_mask must be 30.  status: per world, 0 or why the
// world was not solved (< 0: the block of that mode cannot hold it).
API int32_t dev_solve_worlds(const float *bodies, const int32_t *body_types,
                             const int32_t *body_off,
                             const float *contacts, const int32_t *contact_ints,
                             const int32_t *contact_off,
                             const float *joints, const int32_t *joint_ints,
                             const int32_t *joint_off,
                             const float *sys, uint32_t phase_mask,
                             int32_t num_worlds, int32_t mode,
                             float *bodies_out, float *lambdas,
                             int32_t *status)
{
    if (num_worlds <= 0 || mode < 0 || mode > 3) return -1;
    if (mode != 0 && phase_mask != 30u) return -1;

    const size_t nb = (size_t)body_off[num_worlds];
    const size_t nc = (size_t)contact_off[num_worlds];
    const size_t nj = (size_t)joint_off[num_worlds];
    const size_t nw = (size_t)num_worlds;

    DeviceBuffers dev;
    SolveArgs a {};
    a.bodies = dev.alloc(nb * solver_world::kBodyStride, bodies);
    a.bodyTypes = dev.alloc(nb, body_types);
    a.bodyOff = dev.alloc(nw + 1, body_off);
    a.contacts = dev.alloc(nc * solver_world::kContactStride, contacts);
    a.contactInts = dev.alloc(nc * 3, contact_ints);
    a.contactOff = dev.alloc(nw + 1, contact_off);
    a.joints = dev.alloc(nj * solver_world::kJointStride, joints);
    a.jointInts = dev.alloc(nj * 3, joint_ints);
    a.jointOff = dev.alloc(nw + 1, joint_off);
    a.sys = dev.alloc(nw * 5, sys);
    a.phaseMask = phase_mask;
    a.numWorlds = num_worlds;
    a.bodiesOut = dev.alloc<float>(nb * solver_world::kBodyState);
    a.lambdas = dev.alloc(nc, lambdas);
    a.status = dev.alloc<int32_t>(nw);
    a.work = dev.alloc<solver_world::Body>(nb);
    a.jointRows = dev.alloc<JointConstraint>(nj);
    if (dev.failed) return -2;
    if (hipMemset(a.bodiesOut, 0,
                  sizeof(float) * nb * solver_world::kBodyState) != hipSuccess ||
        hipMemset(a.status, 0xFF, sizeof(int32_t) * nw) != hipSuccess) {
        return -2;
    }

    const uint32_t nwu = (uint32_t)num_worlds;
    if (mode == 0) {
        hipLaunchKernelGGL(solveScalarKernel, dim3((nwu + 63) / 64), dim3(64),
                           0, 0, a);
    } else if (mode == 1) {
        hipLaunchKernelGGL((solveBlockKernel<64, 64>), dim3(nwu), dim3(64),
                           0, 0, a);
    } else if (mode == 2) {
        hipLaunchKernelGGL((solveBlockKernel<32, 32>), dim3((nwu + 1) / 2),
                           dim3(64), 0, 0, a);
    } else {
        hipLaunchKernelGGL((solveBlockKernel<128, 64>), dim3(nwu), dim3(64),
                           0, 0, a);
    }
    if (hipGetLastError() != hipSuccess) return -3;
    if (hipDeviceSynchronize() != hipSuccess) return -3;

    if (hipMemcpy(bodies_out, a.bodiesOut,
                  sizeof(float) * nb * solver_world::kBodyState,
                  hipMemcpyDeviceToHost) != hipSuccess ||
        (nc != 0 && hipMemcpy(lambdas, a.lambdas, sizeof(float) * nc,
                              hipMemcpyDeviceToHost) != hipSuccess) ||
        hipMemcpy(status, a.status, sizeof(int32_t) * nw,
                  hipMemcpyDeviceToHost) != hipSuccess) {
        return -3;
    }
    return 0;
}

// constraintLevels<lpw> over `cases` windows: keys_a / keys_b / levels are
// cases x lpw words, counts[c] <= lpw constraints in window c.  lpw: 64 or 32
// (two windows per wavefront, neighbours share one).
API int32_t dev_constraint_levels(const uint32_t *keys_a,
                                  const uint32_t *keys_b,
                                  const uint32_t *counts, uint32_t cases,
                                  uint32_t lpw, uint32_t *levels)
{
    if (cases == 0 || (lpw != 64 && lpw != 32)) return -1;
    for (uint32_t c = 0; c < cases; c++) {
        if (counts[c] > lpw) return -1;
    }

    DeviceBuffers dev;
    const size_t words = (size_t)cases * lpw;
    const uint32_t *d_a = dev.alloc(words, keys_a);
    const uint32_t *d_b = dev.alloc(words, keys_b);
    const uint32_t *d_counts = dev.alloc((size_t)cases, counts);
    uint32_t *d_levels = dev.alloc<uint32_t>(words);
    if (dev.failed) return -2;

    if (lpw == 64) {
        hipLaunchKernelGGL(levelsKernel<64>, dim3(cases), dim3(64), 0, 0,
                           d_a, d_b, d_counts, cases, d_levels);
    } else {
        hipLaunchKernelGGL(levelsKernel<32>, dim3((cases + 1) / 2), dim3(64),
                           0, 0, d_a, d_b, d_counts, cases, d_levels);
    }
    if (hipGetLastError() != hipSuccess) return -3;
    if (hipDeviceSynchronize() != hipSuccess) return -3;
    return hipMemcpy(levels, d_levels, sizeof(uint32_t) * words,
                     hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}

// wave::nthSetBit<lpw>(masks[c], n) for every n below the mask's population
// count; out: cases x 64 words, 0xFFFFFFFF where n is not below it.  lpw 32:
// only the low 32 bits of a mask may be set.
API int32_t dev_nth_set_bit(const uint64_t *masks, uint32_t cases,
                            uint32_t lpw, uint32_t *out)
{
    if (cases == 0 || (lpw != 64 && lpw != 32)) return -1;
    for (uint32_t c = 0; c < cases; c++) {
        if (lpw == 32 && (masks[c] >> 32) != 0) return -1;
    }

    DeviceBuffers dev;
    const uint64_t *d_masks = dev.alloc((size_t)cases, masks);
    uint32_t *d_out = dev.alloc<uint32_t>((size_t)cases * 64);
    if (dev.failed) return -2;

    if (lpw == 64) {
        hipLaunchKernelGGL(nthSetBitKernel<64>, dim3(cases), dim3(64), 0, 0,
                           d_masks, cases, d_out);
    } else {
        hipLaunchKernelGGL(nthSetBitKernel<32>, dim3(cases), dim3(64), 0, 0,
                           d_masks, cases, d_out);
    }
    if (hipGetLastError() != hipSuccess) return -3;
    if (hipDeviceSynchronize() != hipSuccess) return -3;
    return hipMemcpy(out, d_out, sizeof(uint32_t) * (size_t)cases * 64,
                     hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}

}
