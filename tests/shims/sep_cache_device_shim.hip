// TEST INFRASTRUCTURE.  The remembered separating face of a hull-hull candidate
// (phys_impl/step_narrowphase.inl: sepFaceEntry, sepFaceSeparates, the
// out-parameter of hullHullWaveSAT) run ON THE DEVICE pair by pair, two pairs
// per wavefront on 32 lanes each like the two-worlds-per-wavefront step kernel,
// behind the conventions of phys_device_shim.hip (one hull mesh, pairs of
// transforms, the contact layout of oracle/ref_shims/phys_ref_shim.cpp):
//   * per face of both hulls, its distance from the other hull as one lane
//     computes it for a remembered face, and as the cooperative face query
//     computes it from the hulls staged in LDS;
//   * per pair and per given entry, what the step kernel does with a candidate
//     that carries that entry: the one face first, the cooperative test if it
//     does not separate the pair, the entry the candidate is left with.
#include <madrona/mwhip/user_prelude.hpp>
#pragma clang force_cuda_host_device begin
#include <madrona/physics.hpp>
#include <madrona/physics_assets.hpp>
#include <madrona/physics_loader.hpp>
#pragma clang force_cuda_host_device end

using namespace madrona;
using namespace madrona::phys;
using namespace madrona::phys::narrowphase;

namespace {

constexpr uint32_t kLanes = 32;         // lanes per pair
constexpr uint32_t kFaces = kernels::sepFaceLimit;

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
                                    float *out)
{
    // layout of phys_ref_shim.cpp: has, ref-is-a, numPoints, normal, points
    out[0] = has ? 1.f : 0.f;
    out[1] = has && c.ref.archetype == 1 ? 1.f : 0.f;
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

// lane_dist / coop_dist: num_pairs x 2 (faces of a, of b) x kFaces, NaN where
// there is no such face (coop_dist: or the hulls do not fit the scratch).
// out: num_pairs x num_trials x 28; flags: num_pairs x num_trials, bit 0 too
// big, bit 1 hulls beyond the scratch, bit 2 the entry's face settled the pair,
// bits 8..15 the entry the candidate is left with.
__global__ void __launch_bounds__(64)
sepCacheKernel(const ObjectManager *obj_mgr, const PairIn *pairs,
               uint32_t num_pairs, const uint8_t *entries, uint32_t num_trials,
               float *lane_dist, float *coop_dist, float *out, int32_t *flags)
{
    __shared__ kernels::HullScratch group_scratch[64 / kLanes];

    const uint32_t lane = threadIdx.x % kLanes;
    const uint32_t group = threadIdx.x / kLanes;
    const uint32_t p = blockIdx.x * (64u / kLanes) + group;
    if (p >= num_pairs) {
        return;     // (uniform per 32-lane group, like a half without a world)
    }
    kernels::HullScratch *scratch = &group_scratch[group];

    PairSetup pair {};
    pair.aLoc = Loc { 1, 0 };
    pair.bLoc = Loc { 2, 0 };
    pair.aPrim = &obj_mgr->collisionPrimitives[0];
    pair.bPrim = &obj_mgr->collisionPrimitives[0];
    pair.a = loadTxfm(pairs[p].a);
    pair.b = loadTxfm(pairs[p].b);
    pair.test = NarrowphaseTest::HullHull;
    pair.aabbOverlap = true;

    const float nan = __builtin_nanf("");

    // ---- every face on its own lane, as a remembered face is evaluated ------
    if (lane < kFaces) {
        float of_a = nan, of_b = nan;
        (void)kernels::sepFaceSeparates(pair, kernels::sepFaceOfA | lane, &of_a);
        (void)kernels::sepFaceSeparates(pair, kernels::sepFaceOfB | lane, &of_b);
        lane_dist[((size_t)p * 2 + 0) * kFaces + lane] = of_a;
        lane_dist[((size_t)p * 2 + 1) * kFaces + lane] = of_b;
    }

    // ---- every face as the cooperative face query sees it -------------------
    if (lane < kFaces) {
        coop_dist[((size_t)p * 2 + 0) * kFaces + lane] = nan;
        coop_dist[((size_t)p * 2 + 1) * kFaces + lane] = nan;
    }
    if (kernels::hullsFitScratch<kernels::HullScratch>(pair)) {
        HullState a = kernels::makeHullStateWave<kLanes>(lane,
            pair.aPrim->hull.halfEdgeMesh, pair.a, scratch->hullVerts[0],
            scratch->hullPlanes[0]);
        HullState b = kernels::makeHullStateWave<kLanes>(lane,
            pair.bPrim->hull.halfEdgeMesh, pair.b, scratch->hullVerts[1],
            scratch->hullPlanes[1]);
        kernels::wave::phaseFence();
        if (lane < (uint32_t)a.numFaces()) {
            coop_dist[((size_t)p * 2 + 0) * kFaces + lane] =
                getHullDistanceFromPlane(a.plane(lane), b);
        }
        if (lane < (uint32_t)b.numFaces()) {
            coop_dist[((size_t)p * 2 + 1) * kFaces + lane] =
                getHullDistanceFromPlane(b.plane(lane), a);
        }
        kernels::wave::phaseFence();
    }

    // ---- a candidate that carries `entry`: the step kernel's sequence -------
    for (uint32_t t = 0; t < num_trials; t++) {
        uint32_t entry = entries[(size_t)p * num_trials + t];
        bool settled = false;
        if (entry != 0u) {
            if (kernels::sepFaceSeparates(pair, entry)) {
                settled = true;
            } else {
                entry = 0u;
            }
        }

        ContactConstraint contact {};
        bool has = false;
        bool too_big = false;
        bool large = false;
        if (!settled) {
            uint32_t sep_face = 0;
            has = kernels::hullHullWave<kLanes, true>(lane, pair, scratch,
                &contact, &too_big, kernels::HullHullProf {}, &large, &sep_face);
            if (large) {
                has = kernels::hullHullWaveLazy<kLanes>(lane, pair, scratch,
                                                        &contact, &too_big);
            }
            entry = sep_face;
            kernels::wave::phaseFence();
        }

        if (lane == 0) {
            const size_t at = (size_t)p * num_trials + t;
            storeContact(has, contact, out + at * 28);
            flags[at] = (too_big ? 1 : 0) | (large ? 2 : 0) | (settled ? 4 : 0) |
                (int32_t)(entry << 8);
        }
    }
}

}

extern "C" {

#define API __attribute__((visibility("default")))

API int32_t dev_sep_cache_pairs(const float *verts, uint32_t num_verts,
                                const uint32_t *indices,
                                const uint32_t *face_counts, uint32_t num_faces,
                                const float *pairs, uint32_t num_pairs,
                                const uint8_t *entries, uint32_t num_trials,
                                float *lane_dist, float *coop_dist,
                                float *out, int32_t *flags)
{
    if (num_pairs == 0 || num_trials == 0) return -1;

    imp::SourceMesh mesh {};
    mesh.positions = (math::Vector3 *)verts;
    mesh.indices = (uint32_t *)indices;
    mesh.faceCounts = (uint32_t *)face_counts;
    mesh.numVertices = num_verts;
    mesh.numFaces = num_faces;

    SourceCollisionPrimitive src_prim;
    src_prim.type = CollisionPrimitive::Type::Hull;
    src_prim.hullInput.hullIDX = 0;
    SourceCollisionObject obj {
        Span<const SourceCollisionPrimitive>(&src_prim, 1), 1.f, { 0.5f, 0.5f } };

    StackAlloc tmp_alloc;
    RigidBodyAssets assets;
    CountT num_bytes;
    void *buf = RigidBodyAssets::processRigidBodyAssets(
        Span<const imp::SourceMesh>(&mesh, 1),
        Span<const SourceCollisionObject>(&obj, 1),
        false, tmp_alloc, &assets, &num_bytes);
    if (buf == nullptr) return -1;

    PhysicsLoader loader(ExecMode::CUDA, 4, 0);
    loader.loadRigidBodies(assets);
    free(buf);

    const size_t trials = (size_t)num_pairs * num_trials;
    const size_t dists = (size_t)num_pairs * 2 * kFaces;
    PairIn *d_pairs = nullptr;
    uint8_t *d_entries = nullptr;
    float *d_lane = nullptr, *d_coop = nullptr, *d_out = nullptr;
    int32_t *d_flags = nullptr;
    int32_t rc = -2;
    if (hipMalloc(&d_pairs, sizeof(PairIn) * num_pairs) == hipSuccess &&
        hipMalloc(&d_entries, trials) == hipSuccess &&
        hipMalloc(&d_lane, sizeof(float) * dists) == hipSuccess &&
        hipMalloc(&d_coop, sizeof(float) * dists) == hipSuccess &&
        hipMalloc(&d_out, sizeof(float) * 28 * trials) == hipSuccess &&
        hipMalloc(&d_flags, sizeof(int32_t) * trials) == hipSuccess &&
        hipMemcpy(d_pairs, pairs, sizeof(PairIn) * num_pairs,
                  hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(d_entries, entries, trials,
                  hipMemcpyHostToDevice) == hipSuccess) {
        hipLaunchKernelGGL(sepCacheKernel, dim3((num_pairs + 1) / 2), dim3(64),
                           0, 0, &loader.getObjectManager(), d_pairs, num_pairs,
                           d_entries, num_trials, d_lane, d_coop, d_out, d_flags);
        rc = hipGetLastError() == hipSuccess &&
            hipDeviceSynchronize() == hipSuccess &&
            hipMemcpy(lane_dist, d_lane, sizeof(float) * dists,
                      hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(coop_dist, d_coop, sizeof(float) * dists,
                      hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(out, d_out, sizeof(float) * 28 * trials,
                      hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(flags, d_flags, sizeof(int32_t) * trials,
                      hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
    }
    (void)hipFree(d_pairs);
    (void)hipFree(d_entries);
    (void)hipFree(d_lane);
    (void)hipFree(d_coop);
    (void)hipFree(d_out);
    (void)hipFree(d_flags);
    return rc;
}

}
