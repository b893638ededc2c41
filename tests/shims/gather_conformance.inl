// TEST INFRASTRUCTURE.  The C++ surface of entity gathers (<madrona/mw_gpu.hpp>:
// MWCudaExecutor::makeEntityGather / setStepGather, MWHipEntityGather) named
// member by member.  Included by a plain host translation unit
// (gather_conformance_host.cpp) and by a HIP one compiled for gfx950
// (gather_conformance.hip), each with its own GATHERCONF_NAME; a missing or
// mis-declared member fails the build.  tests/test_gather_abi.py.
#include <madrona/mw_gpu.hpp>

#include <mwhip.h>

#include <type_traits>
#include <utility>

static_assert(MWHIP_ABI_VERSION == 9u, "entity gathers were added under ABI 9, without a bump");
static_assert(sizeof(mwhip_gather_source) == 32, "{ src, num_records, four uint32 }");

namespace {

using madrona::MWCudaExecutor;
using madrona::MWHipEntityGather;
using madrona::Span;
using madrona::py::Tensor;

static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().makeEntityGather(
                                 std::declval<const mwhip_gather_source &>(),
                                 std::declval<Span<const uint32_t>>())),
                             MWHipEntityGather>);
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().setStepGather(
                                 std::declval<const MWHipEntityGather *>(), true)), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipEntityGather &>().compute()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipEntityGather &>().computeAsync()), void>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipEntityGather &>().columnTensor(0u)), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipEntityGather &>().archetypesTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipEntityGather &>().worldsTensor()), Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipEntityGather &>().numHandles()),
                             uint64_t>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipEntityGather &>().handle()),
                             uint64_t>);

}

extern "C" {

#define GATHERCONF_API __attribute__((visibility("default")))
#define GATHERCONF_CAT2(a, b) a##b
#define GATHERCONF_CAT(a, b) GATHERCONF_CAT2(a, b)

// bit 0: default constructible, 1: not copy constructible, 2: not copy
// assignable, 3: move constructible, 4: move assignable
GATHERCONF_API uint32_t GATHERCONF_CAT(GATHERCONF_NAME, _traits)()
{
    return (std::is_default_constructible_v<MWHipEntityGather> ? 1u : 0u) |
        (!std::is_copy_constructible_v<MWHipEntityGather> ? 2u : 0u) |
        (!std::is_copy_assignable_v<MWHipEntityGather> ? 4u : 0u) |
        (std::is_move_constructible_v<MWHipEntityGather> ? 8u : 0u) |
        (std::is_move_assignable_v<MWHipEntityGather> ? 16u : 0u);
}

// the caps of the header, as this translation unit saw them
GATHERCONF_API uint32_t GATHERCONF_CAT(GATHERCONF_NAME, _caps)()
{
    return (uint32_t)MWHIP_GATHER_MAX_COLUMNS << 16 | (uint32_t)MWHIP_MAX_STEP_GATHERS;
}

// every member once, on a caller's executor; returns the bytes of a cell of the
// first listed component times the number of handles (0: something was not as
// it should be)
GATHERCONF_API uint64_t GATHERCONF_CAT(GATHERCONF_NAME, _cycle)(MWCudaExecutor *exec,
                                                              const mwhip_gather_source *source,
                                                              const uint32_t *components,
                                                              uint32_t num_components)
{
    MWHipEntityGather first = exec->makeEntityGather(
        *source, Span<const uint32_t>(components, (madrona::CountT)num_components));
    first.compute();
    first.computeAsync();
    exec->setStepGather(&first, true);
    exec->setStepGather(&first, false);
    MWHipEntityGather second(std::move(first));
    MWHipEntityGather third;
    third = std::move(second);
    const Tensor column = third.columnTensor(0);
    const Tensor archetypes = third.archetypesTensor();
    const Tensor worlds = third.worldsTensor();
    if (third.handle() == 0 || column.devicePtr() == nullptr ||
            archetypes.devicePtr() == nullptr || worlds.devicePtr() == nullptr ||
            column.numDims() != 2 || archetypes.numDims() != 1 || worlds.numDims() != 1 ||
            !column.isOnGPU() || column.dims()[0] != archetypes.dims()[0] ||
            column.dims()[0] != worlds.dims()[0] ||
            column.dims()[0] != (int64_t)third.numHandles()) {
        return 0;
    }
    return (uint64_t)column.dims()[1] * third.numHandles();
}

}
