// A launch that serves several executor objects of one kind:
// its single argument, by value in the kernel-argument segment, holds a count,
// per object the wavefront work items it has and its device-resident plan.
// PlanBatch is that argument for the runtime's own kernels; mwhip_ray_args and
// mwhip_box_args of mwhip.h are the same three fields behind a C ABI, so host
// code (csrc/step_batch.hpp) fills any of them the same way.  A kernel strides
// its wavefronts over batchItems() work items and asks planOfItem() whose each
// one is.  (Which kernels do, and why three spell the two loops out: DESIGN.md
// §24, "the dispatch".)
#pragma once
#include <cstdint>
#include <type_traits>

namespace madrona {
namespace mwhip {

template <typename Plan, uint32_t MAX>
struct PlanBatch {
    uint32_t num_plans;
    uint32_t items[MAX];        // wavefront work items of each object
    const Plan *plans[MAX];
};

#if defined(__HIPCC__)
// Both over any such argument, with constant indices: the arguments stay in
// scalar registers.

// the work items of the whole launch
template <typename Args>
__device__ __forceinline__ uint32_t batchItems(const Args &args)
{
    constexpr uint32_t max = sizeof(args.items) / sizeof(args.items[0]);
    uint32_t total = 0;
#pragma unroll
    for (uint32_t p = 0; p < max; p++) {
        if (p < args.num_plans) total += args.items[p];
    }
    return total;
}

// The plan work item `item` belongs to (null: it is not below batchItems());
// *rel: the item's number among that plan's.
template <typename Args>
__device__ __forceinline__ auto planOfItem(const Args &args, uint32_t item, uint32_t *rel)
{
    constexpr uint32_t max = sizeof(args.items) / sizeof(args.items[0]);
    std::decay_t<decltype(args.plans[0])> plan = nullptr;
    *rel = item;
#pragma unroll
    for (uint32_t p = 0; p < max; p++) {
        if (plan == nullptr && p < args.num_plans) {
            if (*rel < args.items[p]) {
                plan = args.plans[p];
            } else {
                *rel -= args.items[p];
            }
        }
    }
    return plan;
}
#endif

}
}
