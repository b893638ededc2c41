// TEST INFRASTRUCTURE.  The C++ surface of executor snapshots
// (<madrona/mw_gpu.hpp>: MWCudaExecutor::makeSnapshot, MWHipSnapshot) named
// member by member.  Included by a plain host translation unit
// (snapshot_conformance_host.cpp) and by a HIP one compiled for gfx950
// (snapshot_conformance.hip), each with its own SNAPCONF_NAME; a missing or
// mis-declared member fails the build.  tests/test_snapshot_abi.py.
#include <madrona/mw_gpu.hpp>

#include <mwhip.h>

#include <type_traits>
#include <utility>

static_assert(MWHIP_ABI_VERSION >= 9u, "snapshots arrived with ABI 9");

namespace {

using madrona::MWCudaExecutor;
using madrona::MWHipExecutor;
using madrona::MWHipSnapshot;

static_assert(std::is_same_v<MWHipExecutor, MWCudaExecutor>);
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().makeSnapshot()),
                             MWHipSnapshot>);
static_assert(std::is_same_v<decltype(std::declval<MWHipSnapshot &>().save()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipSnapshot &>().restore()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipSnapshot &>().saveAsync()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipSnapshot &>().restoreAsync()), void>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipSnapshot &>().numBytes()),
                             uint64_t>);

}

extern "C" {

#define SNAPCONF_API __attribute__((visibility("default")))
#define SNAPCONF_CAT2(a, b) a##b
#define SNAPCONF_CAT(a, b) SNAPCONF_CAT2(a, b)

// bit 0: default constructible, 1: not copy constructible, 2: not copy
// assignable, 3: move constructible, 4: move assignable
SNAPCONF_API uint32_t SNAPCONF_CAT(SNAPCONF_NAME, _traits)()
{
    return (std::is_default_constructible_v<MWHipSnapshot> ? 1u : 0u) |
        (!std::is_copy_constructible_v<MWHipSnapshot> ? 2u : 0u) |
        (!std::is_copy_assignable_v<MWHipSnapshot> ? 4u : 0u) |
        (std::is_move_constructible_v<MWHipSnapshot> ? 8u : 0u) |
        (std::is_move_assignable_v<MWHipSnapshot> ? 16u : 0u);
}

// every member once, on a caller's executor: save, step nothing, restore;
// returns the bytes the snapshot held
SNAPCONF_API uint64_t SNAPCONF_CAT(SNAPCONF_NAME, _cycle)(MWCudaExecutor *exec)
{
    MWHipSnapshot first = exec->makeSnapshot();
    first.save();
    first.saveAsync();
    first.restoreAsync();
    first.restore();
    MWHipSnapshot second(std::move(first));
    MWHipSnapshot third;
    third = std::move(second);
    return third.handle() != 0 ? third.numBytes() : 0;
}

}
