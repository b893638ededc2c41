// TEST INFRASTRUCTURE.  The C++ surface of entity scatters (<madrona/mw_gpu.hpp>:
// MWCudaExecutor::makeEntityScatter / setStepScatter, MWHipEntityScatter) named
// member by member.  Included by a plain host translation unit
// (scatter_conformance_host.cpp) and by a HIP one compiled for gfx950
// (scatter_conformance.hip), each with its own SCATTERCONF_NAME; a missing or
// mis-declared member fails the build.  tests/test_scatter_abi.py.
#include <madrona/mw_gpu.hpp>

#include <mwhip.h>

#include <type_traits>
#include <utility>

static_assert(MWHIP_ABI_VERSION == 9u, "entity scatters were added under ABI 9, without a bump");
static_assert(sizeof(mwhip_gather_source) == 32, "{ src, num_records, four uint32 }");

namespace {

using madrona::MWCudaExecutor;
using madrona::MWHipEntityScatter;
using madrona::Span;
using madrona::py::Tensor;

static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().makeEntityScatter(
                                 std::declval<const mwhip_gather_source &>(),
                                 std::declval<Span<const uint32_t>>())),
                             MWHipEntityScatter>);
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().setStepScatter(
                                 std::declval<const MWHipEntityScatter *>(), true)), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipEntityScatter &>().apply()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipEntityScatter &>().applyAsync()), void>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipEntityScatter &>().columnTensor(0u)), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipEntityScatter &>().selectTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipEntityScatter &>().archetypesTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipEntityScatter &>().writtenTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipEntityScatter &>().worldsTensor()), Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipEntityScatter &>().numHandles()),
                             uint64_t>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipEntityScatter &>().handle()),
                             uint64_t>);

}

extern "C" {

#define SCATTERCONF_API __attribute__((visibility("default")))
#define SCATTERCONF_CAT2(a, b) a##b
#define SCATTERCONF_CAT(a, b) SCATTERCONF_CAT2(a, b)

// bit 0: default constructible, 1: not copy constructible, 2: not copy
// assignable, 3: move constructible, 4: move assignable
SCATTERCONF_API uint32_t SCATTERCONF_CAT(SCATTERCONF_NAME, _traits)()
{
    return (std::is_default_constructible_v<MWHipEntityScatter> ? 1u : 0u) |
        (!std::is_copy_constructible_v<MWHipEntityScatter> ? 2u : 0u) |
        (!std::is_copy_assignable_v<MWHipEntityScatter> ? 4u : 0u) |
        (std::is_move_constructible_v<MWHipEntityScatter> ? 8u : 0u) |
        (std::is_move_assignable_v<MWHipEntityScatter> ? 16u : 0u);
}

// the caps of the header, as this translation unit saw them
SCATTERCONF_API uint32_t SCATTERCONF_CAT(SCATTERCONF_NAME, _caps)()
{
    return (uint32_t)MWHIP_SCATTER_MAX_COLUMNS << 16 | (uint32_t)MWHIP_MAX_STEP_SCATTERS;
}

// every member once, on a caller's executor; returns the bytes of a cell of the
// first listed component times the number of handles (0: something was not as
// it should be)
SCATTERCONF_API uint64_t SCATTERCONF_CAT(SCATTERCONF_NAME, _cycle)(MWCudaExecutor *exec,
                                                              const mwhip_gather_source *source,
                                                              const uint32_t *components,
                                                              uint32_t num_components)
{
    MWHipEntityScatter first = exec->makeEntityScatter(
        *source, Span<const uint32_t>(components, (madrona::CountT)num_components));
    first.apply();
    first.applyAsync();
    exec->setStepScatter(&first, true);
    exec->setStepScatter(&first, false);
    MWHipEntityScatter second(std::move(first));
    MWHipEntityScatter third;
    third = std::move(second);
    const Tensor column = third.columnTensor(0);
    const Tensor archetypes = third.archetypesTensor();
    const Tensor worlds = third.worldsTensor();
    const Tensor select = third.selectTensor();
    const Tensor written = third.writtenTensor();
    if (third.handle() == 0 || column.devicePtr() == nullptr ||
            archetypes.devicePtr() == nullptr || worlds.devicePtr() == nullptr ||
            select.devicePtr() == nullptr || written.devicePtr() == nullptr ||
            select.numDims() != 1 || written.numDims() != 1 ||
            column.dims()[0] != select.dims()[0] || column.dims()[0] != written.dims()[0] ||
            column.numDims() != 2 || archetypes.numDims() != 1 || worlds.numDims() != 1 ||
            !column.isOnGPU() || column.dims()[0] != archetypes.dims()[0] ||
            column.dims()[0] != worlds.dims()[0] ||
            column.dims()[0] != (int64_t)third.numHandles()) {
        return 0;
    }
    return (uint64_t)column.dims()[1] * third.numHandles();
}

}
