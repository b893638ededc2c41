// TEST INFRASTRUCTURE.  The C++ surface of world reduces (<madrona/mw_gpu.hpp>:
// MWCudaExecutor::makeWorldReduce / setStepReduce, MWHipWorldReduce) named
// member by member.  Included by a plain host translation unit
// (reduce_conformance_host.cpp) and by a HIP one compiled for gfx950
// (reduce_conformance.hip), each with its own REDUCECONF_NAME; a missing or
// mis-declared member fails the build.  tests/test_world_reduce_abi.py.
#include <madrona/mw_gpu.hpp>

#include <mwhip.h>

#include <cstddef>
#include <type_traits>
#include <utility>

static_assert(MWHIP_ABI_VERSION == 9u, "world reduces were added under ABI 9, without a bump");
static_assert(sizeof(mwhip_reduce_term) == 28 && offsetof(mwhip_reduce_term, limit) == 24);

namespace {

using madrona::MWCudaExecutor;
using madrona::MWHipWorldReduce;
using madrona::py::Tensor;

static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().makeWorldReduce(
                                 std::declval<uint32_t>(),
                                 std::declval<const mwhip_reduce_term *>(),
                                 std::declval<uint32_t>())),
                             MWHipWorldReduce>);
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().setStepReduce(
                                 std::declval<const MWHipWorldReduce *>(), true)), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipWorldReduce &>().compute()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipWorldReduce &>().computeAsync()), void>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldReduce &>().termTensor(0u)),
                             Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldReduce &>().countsTensor()),
                             Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldReduce &>().alarmTensor()),
                             Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldReduce &>().numTerms()),
                             uint32_t>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipWorldReduce &>().handle()),
                             uint64_t>);

}

extern "C" {

#define REDUCECONF_API __attribute__((visibility("default")))
#define REDUCECONF_CAT2(a, b) a##b
#define REDUCECONF_CAT(a, b) REDUCECONF_CAT2(a, b)

// bit 0: default constructible, 1: not copy constructible, 2: not copy
// assignable, 3: move constructible, 4: move assignable
REDUCECONF_API uint32_t REDUCECONF_CAT(REDUCECONF_NAME, _traits)()
{
    return (std::is_default_constructible_v<MWHipWorldReduce> ? 1u : 0u) |
        (!std::is_copy_constructible_v<MWHipWorldReduce> ? 2u : 0u) |
        (!std::is_copy_assignable_v<MWHipWorldReduce> ? 4u : 0u) |
        (std::is_move_constructible_v<MWHipWorldReduce> ? 8u : 0u) |
        (std::is_move_assignable_v<MWHipWorldReduce> ? 16u : 0u);
}

// the caps of the header, as this translation unit saw them
REDUCECONF_API uint32_t REDUCECONF_CAT(REDUCECONF_NAME, _caps)()
{
    return (uint32_t)MWHIP_REDUCE_MAX_TERMS << 24 | (uint32_t)MWHIP_REDUCE_MAX_ELEMS << 8 |
        (uint32_t)MWHIP_MAX_STEP_REDUCES;
}

// every member once, on a caller's executor; returns the elements of the first
// term (0: something was not as it should be)
REDUCECONF_API uint32_t REDUCECONF_CAT(REDUCECONF_NAME, _cycle)(MWCudaExecutor *exec,
                                                             uint32_t archetype,
                                                             const mwhip_reduce_term *terms,
                                                             uint32_t num_terms)
{
    MWHipWorldReduce first = exec->makeWorldReduce(archetype, terms, num_terms);
    first.compute();
    first.computeAsync();
    exec->setStepReduce(&first, true);
    exec->setStepReduce(&first, false);
    MWHipWorldReduce second(std::move(first));
    MWHipWorldReduce third;
    third = std::move(second);
    const Tensor term = third.termTensor(0);
    const Tensor counts = third.countsTensor();
    const Tensor alarm = third.alarmTensor();
    if (third.handle() == 0 || third.numTerms() != num_terms || term.devicePtr() == nullptr ||
            counts.devicePtr() == nullptr || alarm.devicePtr() == nullptr ||
            alarm.devicePtr() == counts.devicePtr() || term.numDims() != 2 ||
            counts.numDims() != 1 || alarm.numDims() != 1 || !term.isOnGPU() ||
            term.dims()[0] != counts.dims()[0] || alarm.dims()[0] != counts.dims()[0]) {
        return 0;
    }
    // every term's tensor is in its result type: Float32 for SUM / MIN / MAX
    // of F32 and for ABSMAX, Int32 otherwise
    for (uint32_t i = 0; i < num_terms; i++) {
        const Tensor each = third.termTensor(i);
        const bool is_float = terms[i].dtype == MWHIP_REDUCE_F32 &&
            terms[i].op <= MWHIP_REDUCE_ABSMAX;
        if (each.devicePtr() == nullptr || each.numDims() != 2 ||
                each.dims()[0] != counts.dims()[0] ||
                each.dims()[1] != (int64_t)terms[i].num_elems ||
                each.type() != (is_float ? madrona::py::TensorElementType::Float32 :
                                madrona::py::TensorElementType::Int32)) {
            return 0;
        }
    }
    return (uint32_t)term.dims()[1];
}

}
