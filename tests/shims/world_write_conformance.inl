// TEST INFRASTRUCTURE.  The C++ surface of world writes (<madrona/mw_gpu.hpp>:
// MWCudaExecutor::makeWorldWrite / setStepWrite, MWHipWorldWrite) named member
// by member.  Included by a plain host translation unit
// (world_write_conformance_host.cpp) and by a HIP one compiled for gfx950
// (world_write_conformance.hip), each with its own WRITECONF_NAME; a missing or
// mis-declared member fails the build.  tests/test_world_write_abi.py.
#include <madrona/mw_gpu.hpp>

#include <mwhip.h>

#include <type_traits>
#include <utility>

static_assert(MWHIP_ABI_VERSION == 9u, "world writes were added under ABI 9, without a bump");

namespace {

using madrona::MWCudaExecutor;
using madrona::MWHipWorldWrite;
using madrona::Span;
using madrona::py::Tensor;

static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().makeWorldWrite(
                                 std::declval<uint32_t>(),
                                 std::declval<Span<const uint32_t>>(),
                                 std::declval<uint32_t>())),
                             MWHipWorldWrite>);
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().setStepWrite(
                                 std::declval<const MWHipWorldWrite *>(), true)), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipWorldWrite &>().apply()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipWorldWrite &>().applyAsync()), void>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldWrite &>().columnTensor(0u)),
                             Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldWrite &>().takeTensor()),
                             Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldWrite &>().countsTensor()),
                             Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldWrite &>().maxRows()),
                             uint32_t>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldWrite &>().handle()),
                             uint64_t>);

}

extern "C" {

#define WRITECONF_API __attribute__((visibility("default")))
#define WRITECONF_CAT2(a, b) a##b
#define WRITECONF_CAT(a, b) WRITECONF_CAT2(a, b)

// bit 0: default constructible, 1: not copy constructible, 2: not copy
// assignable, 3: move constructible, 4: move assignable
WRITECONF_API uint32_t WRITECONF_CAT(WRITECONF_NAME, _traits)()
{
    return (std::is_default_constructible_v<MWHipWorldWrite> ? 1u : 0u) |
        (!std::is_copy_constructible_v<MWHipWorldWrite> ? 2u : 0u) |
        (!std::is_copy_assignable_v<MWHipWorldWrite> ? 4u : 0u) |
        (std::is_move_constructible_v<MWHipWorldWrite> ? 8u : 0u) |
        (std::is_move_assignable_v<MWHipWorldWrite> ? 16u : 0u);
}

// the caps of the header, as this translation unit saw them
WRITECONF_API uint32_t WRITECONF_CAT(WRITECONF_NAME, _caps)()
{
    return (uint32_t)MWHIP_WRITE_MAX_COLUMNS << 16 | (uint32_t)MWHIP_MAX_STEP_WRITES;
}

// every member once, on a caller's executor (take is zero: nothing is written);
// returns the bytes of a cell of the first listed column times max_rows (0:
// something was not as it should be)
WRITECONF_API uint32_t WRITECONF_CAT(WRITECONF_NAME, _cycle)(MWCudaExecutor *exec,
                                                          uint32_t archetype,
                                                          const uint32_t *components,
                                                          uint32_t num_components,
                                                          uint32_t max_rows)
{
    MWHipWorldWrite first = exec->makeWorldWrite(
        archetype, Span<const uint32_t>(components, (madrona::CountT)num_components), max_rows);
    first.apply();
    first.applyAsync();
    exec->setStepWrite(&first, true);
    exec->setStepWrite(&first, false);
    MWHipWorldWrite second(std::move(first));
    MWHipWorldWrite third;
    third = std::move(second);
    const Tensor column = third.columnTensor(0);
    const Tensor take = third.takeTensor();
    const Tensor counts = third.countsTensor();
    if (third.handle() == 0 || column.devicePtr() == nullptr || take.devicePtr() == nullptr ||
            counts.devicePtr() == nullptr || take.devicePtr() == counts.devicePtr() ||
            column.numDims() != 3 || take.numDims() != 1 || counts.numDims() != 1 ||
            !column.isOnGPU() || column.dims()[0] != counts.dims()[0] ||
            take.dims()[0] != counts.dims()[0] || column.dims()[1] != (int64_t)max_rows) {
        return 0;
    }
    return (uint32_t)column.dims()[2] * third.maxRows();
}

}
