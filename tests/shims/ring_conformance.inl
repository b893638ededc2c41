// TEST INFRASTRUCTURE.  The C++ surface of the device-resident rings
// (<madrona/mw_gpu.hpp>: MWCudaExecutor::setInputRing, setOutputRing,
// outputRingRecorded) named member by member.  Included by a plain host
// translation unit (ring_conformance_host.cpp) and by a HIP one compiled for
// gfx950 (ring_conformance.hip), each with its own RINGCONF_NAME; a missing or
// mis-declared member fails the build.  tests/test_output_ring_abi.py.
#include <madrona/mw_gpu.hpp>

#include <mwhip.h>

#include <type_traits>
#include <utility>

static_assert(MWHIP_ABI_VERSION == 9u, "the output rings were added under ABI 9");
static_assert(MWHIP_MAX_OUTPUT_RINGS == 16);
static_assert(MWHIP_RING_ON_STEP == 0u && MWHIP_RING_ON_RENDER == 1u);

namespace {

using madrona::MWCudaExecutor;

using SetInputRing = void (MWCudaExecutor::*)(void *, const void *, uint64_t, uint32_t);
using SetOutputRing = void (MWCudaExecutor::*)(const void *, void *, uint64_t, uint32_t,
                                               bool);
using OutputRingRecorded = uint64_t (MWCudaExecutor::*)(const void *, bool);
static_assert(std::is_same_v<decltype(&MWCudaExecutor::setInputRing), SetInputRing>);
static_assert(std::is_same_v<decltype(&MWCudaExecutor::setOutputRing), SetOutputRing>);
static_assert(std::is_same_v<decltype(&MWCudaExecutor::outputRingRecorded),
                             OutputRingRecorded>);
// on_render defaults to false
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().setOutputRing(
                                 nullptr, nullptr, 0, 0)), void>);
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().outputRingRecorded(
                                 nullptr)), uint64_t>);

}

extern "C" {

#define RINGCONF_API __attribute__((visibility("default")))
#define RINGCONF_CAT2(a, b) a##b
#define RINGCONF_CAT(a, b) RINGCONF_CAT2(a, b)

// the values of the three macros, packed: rings << 16 | on_render << 8 | on_step
RINGCONF_API uint32_t RINGCONF_CAT(RINGCONF_NAME, _macros)()
{
    return (uint32_t)MWHIP_MAX_OUTPUT_RINGS << 16 | MWHIP_RING_ON_RENDER << 8 |
        MWHIP_RING_ON_STEP;
}

// every member once, on a caller's executor: an output ring of `slots` slots on
// `src`, an input ring on `dst`, both removed again; returns what
// outputRingRecorded said in between
RINGCONF_API uint64_t RINGCONF_CAT(RINGCONF_NAME, _cycle)(
    MWCudaExecutor *exec, const void *src, void *out_ring, void *dst,
    const void *in_ring, uint64_t slot_bytes, uint32_t slots)
{
    exec->setOutputRing(src, out_ring, slot_bytes, slots);
    exec->setOutputRing(src, out_ring, slot_bytes, slots, true);
    exec->setInputRing(dst, in_ring, slot_bytes, slots);
    const uint64_t recorded =
        exec->outputRingRecorded(src) + exec->outputRingRecorded(src, true);
    exec->setInputRing(dst, nullptr, 0, 0);
    exec->setOutputRing(src, nullptr, 0, 0, true);
    exec->setOutputRing(src, nullptr, 0, 0);
    return recorded;
}

}
