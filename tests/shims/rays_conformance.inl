// TEST INFRASTRUCTURE.  The C++ surface of ray queries (<madrona/mw_gpu.hpp>:
// MWCudaExecutor::makeRayQuery / setStepRays, MWHipRayQuery) named member by
// member.  Included by a plain host translation unit (rays_conformance_host.cpp)
// and by a HIP one compiled for gfx950 (rays_conformance.hip), each with its own
// RAYSCONF_NAME; a missing or mis-declared member fails the build.
// tests/test_ray_query_abi.py.
#include <madrona/mw_gpu.hpp>

#include <mwhip.h>

#include <type_traits>
#include <utility>

static_assert(MWHIP_ABI_VERSION == 9u, "ray queries were added under ABI 9, without a bump");
static_assert(sizeof(mwhip_ray_source) == 16, "{ src, two uint32 }");
static_assert(sizeof(mwhip_rays_desc) == 64, "{ four uint32, three sources }");
static_assert(sizeof(mwhip_ray_plan) == 112 && sizeof(mwhip_ray_args) == 56,
              "what the runtime and the simulator's kernel share");

namespace {

using madrona::MWCudaExecutor;
using madrona::MWHipRayQuery;
using madrona::py::Tensor;

static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().makeRayQuery(
                                 std::declval<const mwhip_rays_desc &>())), MWHipRayQuery>);
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().setStepRays(
                                 std::declval<const MWHipRayQuery *>(), true)), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipRayQuery &>().compute()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipRayQuery &>().computeAsync()), void>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipRayQuery &>().worldsTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipRayQuery &>().originsTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipRayQuery &>().directionsTensor()), Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipRayQuery &>().tMaxTensor()), Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipRayQuery &>().hitTTensor()), Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipRayQuery &>().hitsTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipRayQuery &>().normalsTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipRayQuery &>().statusTensor()), Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipRayQuery &>().handleSource()),
                             mwhip_gather_source>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipRayQuery &>().numFans()), uint64_t>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipRayQuery &>().numRays()), uint64_t>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipRayQuery &>().handle()), uint64_t>);

}

extern "C" {

#define RAYSCONF_API __attribute__((visibility("default")))
#define RAYSCONF_CAT2(a, b) a##b
#define RAYSCONF_CAT(a, b) RAYSCONF_CAT2(a, b)

// bit 0: default constructible, 1: not copy constructible, 2: not copy
// assignable, 3: move constructible, 4: move assignable
RAYSCONF_API uint32_t RAYSCONF_CAT(RAYSCONF_NAME, _traits)()
{
    return (std::is_default_constructible_v<MWHipRayQuery> ? 1u : 0u) |
        (!std::is_copy_constructible_v<MWHipRayQuery> ? 2u : 0u) |
        (!std::is_copy_assignable_v<MWHipRayQuery> ? 4u : 0u) |
        (std::is_move_constructible_v<MWHipRayQuery> ? 8u : 0u) |
        (std::is_move_assignable_v<MWHipRayQuery> ? 16u : 0u);
}

// the caps and codes of the header, as this translation unit saw them
RAYSCONF_API uint32_t RAYSCONF_CAT(RAYSCONF_NAME, _caps)()
{
    return (uint32_t)MWHIP_MAX_STEP_RAYS << 16 | (uint32_t)MWHIP_RAYS_NUM_BUFS << 8 |
        (uint32_t)(MWHIP_RAYS_HIT - MWHIP_RAYS_BAD_RAY);
}

// every member once, on a caller's executor and a query whose world and origin
// are owned; returns rays x fans (0: something was not as it should be)
RAYSCONF_API uint64_t RAYSCONF_CAT(RAYSCONF_NAME, _cycle)(MWCudaExecutor *exec,
                                                          const mwhip_rays_desc *desc)
{
    MWHipRayQuery first = exec->makeRayQuery(*desc);
    first.compute();
    first.computeAsync();
    exec->setStepRays(&first, true);
    exec->setStepRays(&first, false);
    MWHipRayQuery second(std::move(first));
    MWHipRayQuery third;
    third = std::move(second);
    const Tensor worlds = third.worldsTensor();
    const Tensor origins = third.originsTensor();
    const Tensor directions = third.directionsTensor();
    const Tensor t_max = third.tMaxTensor();
    const Tensor hit_t = third.hitTTensor();
    const Tensor hits = third.hitsTensor();
    const Tensor normals = third.normalsTensor();
    const Tensor status = third.statusTensor();
    const mwhip_gather_source source = third.handleSource();
    if (third.handle() == 0 || worlds.numDims() != 1 || origins.numDims() != 2 ||
            directions.numDims() != 2 || t_max.numDims() != 1 || hit_t.numDims() != 1 ||
            hits.numDims() != 2 || normals.numDims() != 2 || status.numDims() != 1 ||
            !status.isOnGPU() || worlds.dims()[0] != (int64_t)third.numFans() ||
            origins.dims()[0] != (int64_t)third.numFans() || origins.dims()[1] != 3 ||
            directions.dims()[0] != (int64_t)third.numRays() || hits.dims()[1] != 2 ||
            status.dims()[0] != (int64_t)third.numRays() || source.src != hits.devicePtr() ||
            source.num_records != third.numRays() || source.record_bytes != 8u ||
            source.handles_per_record != 1u) {
        return 0;
    }
    return third.numRays() * third.numFans();
}

}
