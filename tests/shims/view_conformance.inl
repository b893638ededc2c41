// TEST INFRASTRUCTURE.  The C++ surface of world views (<madrona/mw_gpu.hpp>:
// MWCudaExecutor::makeWorldView / setStepView, MWHipWorldView) named member by
// member.  Included by a plain host translation unit
// (view_conformance_host.cpp) and by a HIP one compiled for gfx950
// (view_conformance.hip), each with its own VIEWCONF_NAME; a missing or
// mis-declared member fails the build.  tests/test_world_view_abi.py.
#include <madrona/mw_gpu.hpp>

#include <mwhip.h>

#include <type_traits>
#include <utility>

static_assert(MWHIP_ABI_VERSION == 9u, "world views were added under ABI 9, without a bump");

namespace {

using madrona::MWCudaExecutor;
using madrona::MWHipWorldView;
using madrona::Span;
using madrona::py::Tensor;

static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().makeWorldView(
                                 std::declval<uint32_t>(),
                                 std::declval<Span<const uint32_t>>(),
                                 std::declval<uint32_t>())),
                             MWHipWorldView>);
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().setStepView(
                                 std::declval<const MWHipWorldView *>(), true)), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipWorldView &>().compute()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipWorldView &>().computeAsync()), void>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldView &>().columnTensor(0u)),
                             Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldView &>().countsTensor()),
                             Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldView &>().maxRows()),
                             uint32_t>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldView &>().handle()),
                             uint64_t>);

}

extern "C" {

#define VIEWCONF_API __attribute__((visibility("default")))
#define VIEWCONF_CAT2(a, b) a##b
#define VIEWCONF_CAT(a, b) VIEWCONF_CAT2(a, b)

// bit 0: default constructible, 1: not copy constructible, 2: not copy
// assignable, 3: move constructible, 4: move assignable
VIEWCONF_API uint32_t VIEWCONF_CAT(VIEWCONF_NAME, _traits)()
{
    return (std::is_default_constructible_v<MWHipWorldView> ? 1u : 0u) |
        (!std::is_copy_constructible_v<MWHipWorldView> ? 2u : 0u) |
        (!std::is_copy_assignable_v<MWHipWorldView> ? 4u : 0u) |
        (std::is_move_constructible_v<MWHipWorldView> ? 8u : 0u) |
        (std::is_move_assignable_v<MWHipWorldView> ? 16u : 0u);
}

// the caps of the header, as this translation unit saw them
VIEWCONF_API uint32_t VIEWCONF_CAT(VIEWCONF_NAME, _caps)()
{
    return (uint32_t)MWHIP_VIEW_MAX_COLUMNS << 16 | (uint32_t)MWHIP_MAX_STEP_VIEWS;
}

// every member once, on a caller's executor; returns the bytes of a cell of the
// first listed column times max_rows (0: something was not as it should be)
VIEWCONF_API uint32_t VIEWCONF_CAT(VIEWCONF_NAME, _cycle)(MWCudaExecutor *exec,
                                                        uint32_t archetype,
                                                        const uint32_t *components,
                                                        uint32_t num_components,
                                                        uint32_t max_rows)
{
    MWHipWorldView first = exec->makeWorldView(
        archetype, Span<const uint32_t>(components, (madrona::CountT)num_components), max_rows);
    first.compute();
    first.computeAsync();
    exec->setStepView(&first, true);
    exec->setStepView(&first, false);
    MWHipWorldView second(std::move(first));
    MWHipWorldView third;
    third = std::move(second);
    const Tensor column = third.columnTensor(0);
    const Tensor counts = third.countsTensor();
    if (third.handle() == 0 || column.devicePtr() == nullptr || counts.devicePtr() == nullptr ||
            column.numDims() != 3 || counts.numDims() != 1 || !column.isOnGPU() ||
            column.dims()[0] != counts.dims()[0] || column.dims()[1] != (int64_t)max_rows) {
        return 0;
    }
    return (uint32_t)column.dims()[2] * third.maxRows();
}

}
