// TEST INFRASTRUCTURE.  The C++ surface of box queries (<madrona/mw_gpu.hpp>:
// MWCudaExecutor::makeBoxQuery / setStepBoxes, MWHipBoxQuery) named member by
// member.  Included by a plain host translation unit (boxes_conformance_host.cpp)
// and by a HIP one compiled for gfx950 (boxes_conformance.hip), each with its own
// BOXESCONF_NAME; a missing or mis-declared member fails the build.
// tests/test_box_query_abi.py.
#include <madrona/mw_gpu.hpp>

#include <mwhip.h>

#include <type_traits>
#include <utility>

static_assert(MWHIP_ABI_VERSION == 9u, "box queries were added under ABI 9, without a bump");
static_assert(sizeof(mwhip_boxes_desc) == 72, "{ six uint32, three sources }");
static_assert(sizeof(mwhip_box_plan) == 104 && sizeof(mwhip_box_args) == 56,
              "what the runtime and the simulator's kernel share");
// (the structs ray queries added stay as simulator libraries were compiled
// against them)
static_assert(sizeof(mwhip_ray_source) == 16 && sizeof(mwhip_ray_plan) == 112 &&
              sizeof(mwhip_ray_args) == 56);

namespace {

using madrona::MWCudaExecutor;
using madrona::MWHipBoxQuery;
using madrona::py::Tensor;

static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().makeBoxQuery(
                                 std::declval<const mwhip_boxes_desc &>())), MWHipBoxQuery>);
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().setStepBoxes(
                                 std::declval<const MWHipBoxQuery *>(), true)), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipBoxQuery &>().compute()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipBoxQuery &>().computeAsync()), void>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipBoxQuery &>().worldsTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipBoxQuery &>().centresTensor()), Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipBoxQuery &>().loTensor()), Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipBoxQuery &>().hiTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipBoxQuery &>().statusTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipBoxQuery &>().countsTensor()), Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipBoxQuery &>().hitsTensor()), Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipBoxQuery &>().handleSource()),
                             mwhip_gather_source>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipBoxQuery &>().numBundles()), uint64_t>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipBoxQuery &>().numBoxes()), uint64_t>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipBoxQuery &>().maxHits()), uint64_t>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipBoxQuery &>().handle()), uint64_t>);

}

extern "C" {

#define BOXESCONF_API __attribute__((visibility("default")))
#define BOXESCONF_CAT2(a, b) a##b
#define BOXESCONF_CAT(a, b) BOXESCONF_CAT2(a, b)

// bit 0: default constructible, 1: not copy constructible, 2: not copy
// assignable, 3: move constructible, 4: move assignable
BOXESCONF_API uint32_t BOXESCONF_CAT(BOXESCONF_NAME, _traits)()
{
    return (std::is_default_constructible_v<MWHipBoxQuery> ? 1u : 0u) |
        (!std::is_copy_constructible_v<MWHipBoxQuery> ? 2u : 0u) |
        (!std::is_copy_assignable_v<MWHipBoxQuery> ? 4u : 0u) |
        (std::is_move_constructible_v<MWHipBoxQuery> ? 8u : 0u) |
        (std::is_move_assignable_v<MWHipBoxQuery> ? 16u : 0u);
}

// the caps and codes of the header, as this translation unit saw them
BOXESCONF_API uint32_t BOXESCONF_CAT(BOXESCONF_NAME, _caps)()
{
    return (uint32_t)MWHIP_MAX_STEP_BOXES << 16 | (uint32_t)MWHIP_BOXES_NUM_BUFS << 8 |
        (uint32_t)MWHIP_BOXES_PACKED << 4 | (uint32_t)(MWHIP_BOXES_OK - MWHIP_BOXES_BAD_BOX);
}

// every member once, on a caller's executor and a query whose world and centre
// are owned; returns boxes x hits x bundles (0: something was not as it should
// be)
BOXESCONF_API uint64_t BOXESCONF_CAT(BOXESCONF_NAME, _cycle)(MWCudaExecutor *exec,
                                                             const mwhip_boxes_desc *desc)
{
    MWHipBoxQuery first = exec->makeBoxQuery(*desc);
    first.compute();
    first.computeAsync();
    exec->setStepBoxes(&first, true);
    exec->setStepBoxes(&first, false);
    MWHipBoxQuery second(std::move(first));
    MWHipBoxQuery third;
    third = std::move(second);
    const Tensor worlds = third.worldsTensor();
    const Tensor centres = third.centresTensor();
    const Tensor lo = third.loTensor();
    const Tensor hi = third.hiTensor();
    const Tensor status = third.statusTensor();
    const Tensor counts = third.countsTensor();
    const Tensor hits = third.hitsTensor();
    const mwhip_gather_source source = third.handleSource();
    if (third.handle() == 0 || worlds.numDims() != 1 || centres.numDims() != 2 ||
            lo.numDims() != 2 || hi.numDims() != 2 || status.numDims() != 1 ||
            counts.numDims() != 1 || hits.numDims() != 3 || !status.isOnGPU() ||
            worlds.dims()[0] != (int64_t)third.numBundles() ||
            centres.dims()[0] != (int64_t)third.numBundles() || centres.dims()[1] != 3 ||
            lo.dims()[0] != (int64_t)third.numBoxes() || hi.dims()[1] != 3 ||
            hits.dims()[0] != (int64_t)third.numBoxes() ||
            hits.dims()[1] != (int64_t)third.maxHits() || hits.dims()[2] != 2 ||
            counts.dims()[0] != (int64_t)third.numBoxes() || source.src != hits.devicePtr() ||
            source.num_records != third.numBoxes() * third.maxHits() ||
            source.record_bytes != 8u || source.handles_per_record != 1u) {
        return 0;
    }
    return third.numBoxes() * third.maxHits() * third.numBundles();
}

}
