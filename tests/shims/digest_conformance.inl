// TEST INFRASTRUCTURE.  The C++ surface of state digests
// (<madrona/mw_gpu.hpp>: MWCudaExecutor::makeDigest / setStepDigest,
// MWHipDigest, DigestColumn) named member by member.  Included by a plain host
// translation unit (digest_conformance_host.cpp) and by a HIP one compiled for
// gfx950 (digest_conformance.hip), each with its own DIGCONF_NAME; a missing or
// mis-declared member fails the build.  tests/test_digest_abi.py.
#include <madrona/mw_gpu.hpp>

#include <mwhip.h>

#include <type_traits>
#include <utility>

static_assert(MWHIP_ABI_VERSION >= 9u, "digests were added under ABI 9");

namespace {

using madrona::DigestColumn;
using madrona::MWCudaExecutor;
using madrona::MWHipDigest;
using madrona::Span;

static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().makeDigest(
                                 std::declval<Span<const DigestColumn>>())),
                             MWHipDigest>);
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().setStepDigest(
                                 std::declval<const MWHipDigest *>())), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipDigest &>().compute()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipDigest &>().computeAsync()), void>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipDigest &>().devicePtr()),
                             void *>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipDigest &>().numGroups()),
                             uint32_t>);
static_assert(sizeof(DigestColumn) == 8 &&
              offsetof(DigestColumn, archetypeID) == offsetof(mwhip_digest_column, archetype_id) &&
              offsetof(DigestColumn, componentID) == offsetof(mwhip_digest_column, component_id));

}

extern "C" {

#define DIGCONF_API __attribute__((visibility("default")))
#define DIGCONF_CAT2(a, b) a##b
#define DIGCONF_CAT(a, b) DIGCONF_CAT2(a, b)

// bit 0: default constructible, 1: not copy constructible, 2: not copy
// assignable, 3: move constructible, 4: move assignable
DIGCONF_API uint32_t DIGCONF_CAT(DIGCONF_NAME, _traits)()
{
    return (std::is_default_constructible_v<MWHipDigest> ? 1u : 0u) |
        (!std::is_copy_constructible_v<MWHipDigest> ? 2u : 0u) |
        (!std::is_copy_assignable_v<MWHipDigest> ? 4u : 0u) |
        (std::is_move_constructible_v<MWHipDigest> ? 8u : 0u) |
        (std::is_move_assignable_v<MWHipDigest> ? 16u : 0u);
}

// the caps of the header, as this translation unit saw them
DIGCONF_API uint32_t DIGCONF_CAT(DIGCONF_NAME, _caps)()
{
    return (uint32_t)MWHIP_DIGEST_MAX_COLUMNS << 16 | (uint32_t)MWHIP_DIGEST_MAX_GROUPS;
}

// every member once, on a caller's executor and plan; returns the groups
DIGCONF_API uint32_t DIGCONF_CAT(DIGCONF_NAME, _cycle)(MWCudaExecutor *exec,
                                                      const DigestColumn *columns,
                                                      uint32_t num_columns)
{
    MWHipDigest first =
        exec->makeDigest(Span<const DigestColumn>(columns, (madrona::CountT)num_columns));
    first.compute();
    first.computeAsync();
    exec->setStepDigest(&first);
    exec->setStepDigest(nullptr);
    MWHipDigest second(std::move(first));
    MWHipDigest third;
    third = std::move(second);
    return third.handle() != 0 && third.devicePtr() != nullptr ? third.numGroups() : 0;
}

}
