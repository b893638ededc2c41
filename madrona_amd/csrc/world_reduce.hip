// libmadrona_hip.so -- world reductions: one number per world, element and term
// about one table -- sums, extrema, counts and an alarm word -- written where
// the table is (mwhip_reduce_*, include/mwhip.h; DESIGN.md §28;
// madrona_amd/reduce_ref.py is the definition).
//
// A reduce owns a device-resident PLAN -- the table header and, per element of
// the terms' elements listed one after another, the header slot its column's
// base address is read from (the sort swaps a column with its twin), the cell
// bytes, where the element is in the cell, what to do with it and where its
// result goes -- and one allocation that holds the results, the counts and the
// alarms.  Row counts, the sorted
// prefix and column bases are read on the device when the kernel runs.
//   worldReduceKernel  a TEAM of T = min(64, next power of two >= elements of
//                      the plan) lanes owns one world, a wavefront 64 / T
//                      consecutive worlds; wavefronts stride over the (reduce,
//                      64 / T worlds) items of up to MWHIP_MAX_STEP_REDUCES
//                      reduces passed by value.
// A lane owns ELEMENTS (of the plan's list of all terms' elements: lane t those
// numbered t, t + 64, ... -- up to four), and the team walks its world's rows
// in ascending order, so every accumulator meets its values in row order: the
// float sum is the sequential one of the definition.  A team
//   1. reads the WorldID cells of its world's range of the sorted prefix (a
//      hint, world_team.hpp) and counts those equal to w;
//   2. if all of them are: walks the range in row order, no further tests, the
//      loads of eight rows in flight together; if not
//      (rows destroyed in place): goes through it again T rows at a time and
//      walks the rows a ballot masked to the team found, lowest first;
//   3. scans [sortedRows, numRows) the same way;
//   4. stores its results, count[w] and alarm[w] (a ballot of the lanes whose
//      alarm terms tripped, masked to the team).
// A team writes nothing but its own world's outputs, with plain vector stores:
// no atomics, no spin-waits, no workgroup waits for another, no LDS.
#include "exec_internal.hpp"
#include "world_team.hpp"

#include <cstring>

namespace {

constexpr uint32_t kReduceThreads = 256;
constexpr uint32_t kReduceWaves = kReduceThreads / 64u;
constexpr uint32_t kReduceSlots = MWHIP_REDUCE_MAX_ELEMS / 64u;    // elements per lane

// what an accumulator does with a value: (op, class of the result type)
enum ReduceKind : uint32_t {
    kNone = 0,
    kSumF, kSumI,
    kMinF, kMinI, kMinU,
    kMaxF, kMaxI, kMaxU,
    kAbsMax,
    kNonZeroF, kNonZeroI,
    kNonFinite,
};
constexpr uint32_t kKindMask = 0xFFu;
constexpr uint32_t kLoadU8 = 0x100u;        // the element is one byte, widened

// One per element of the plan, everything its lane needs in one place (the
// lane's first loads are one level deep, next to those of the table header)
struct ReducePlanElem {
    void *const *slot;      // &hdr->columns[c] on the device
    uint32_t *out;          // the element's result of world 0; world w: out[w * outStride]
    uint32_t byteOffset;    // of the element in its cell
    uint32_t cellBytes;
    uint32_t kind;          // ReduceKind | kLoadU8
    uint32_t identity;      // the accumulator's first value (bits)
    uint32_t outStride;     // the elements of its term
    uint32_t alarm;         // 0 / 1
    float limit;
    uint32_t pad_;
};

struct ReducePlan {
    const TableHdr *hdr;    // on the device
    int32_t *counts;        // [numWorlds]
    int32_t *alarm;         // [numWorlds]
    uint32_t numWorlds;
    uint32_t numElems;      // of all terms, 1 .. MWHIP_REDUCE_MAX_ELEMS
    uint32_t numTerms;
    uint32_t teamLanes;     // T: a power of two, 1 .. 64
    ReducePlanElem elems[MWHIP_REDUCE_MAX_ELEMS];
};

// a term while its plan is made (host only)
struct ReduceTermInfo {
    uint32_t column;        // in the list of distinct components
    uint32_t byteOffset;
    uint32_t numElems;
    uint32_t firstElem;     // of the plan's element list
    uint32_t kind;
    uint32_t elemBytes;
    uint32_t alarm;
    uint32_t identity;
    float limit;
};

// by value in the kernel-argument segment, like ViewArgs
using ReduceArgs = madrona::mwhip::PlanBatch<ReducePlan, MWHIP_MAX_STEP_REDUCES>;

using madrona::mwhip::GlobalU32;
using madrona::mwhip::GlobalU8;

// one element of one lane
struct ReduceSlot {
    const char *src;        // element of row 0
    uint32_t stride;        // cell bytes
    uint32_t kind;          // kNone: the lane has no such element
    uint32_t acc;           // bits
};

__device__ inline uint32_t loadElem(const ReduceSlot &s, int32_t r)
{
    const uint64_t p = (uint64_t)s.src + (uint64_t)(uint32_t)r * s.stride;
    if ((s.kind & kLoadU8) != 0u) {
        return (uint32_t)*(const GlobalU8 *)p;
    }
    return *(const GlobalU32 *)p;
}

// (plain comparisons and one fp32 add, in the order given: the definition)
__device__ inline uint32_t accumulate(uint32_t kind, uint32_t acc, uint32_t x)
{
    switch (kind & kKindMask) {
    case kSumF: return __float_as_uint(__uint_as_float(acc) + __uint_as_float(x));
    case kSumI: return acc + x;
    case kMinF: return __uint_as_float(x) < __uint_as_float(acc) ? x : acc;
    case kMinI: return (int32_t)x < (int32_t)acc ? x : acc;
    case kMinU: return x < acc ? x : acc;
    case kMaxF: return __uint_as_float(x) > __uint_as_float(acc) ? x : acc;
    case kMaxI: return (int32_t)x > (int32_t)acc ? x : acc;
    case kMaxU: return x > acc ? x : acc;
    case kAbsMax: {
        const uint32_t a = x & 0x7FFFFFFFu;
        return __uint_as_float(a) > __uint_as_float(acc) ? a : acc;
    }
    case kNonZeroF: return acc + ((x & 0x7FFFFFFFu) != 0u ? 1u : 0u);
    case kNonZeroI: return acc + (x != 0u ? 1u : 0u);
    case kNonFinite: return acc + ((x & 0x7F800000u) == 0x7F800000u ? 1u : 0u);
    default: return acc;
    }
}

constexpr uint32_t kReduceGroup = 8;      // rows whose loads are in flight together

// the first n of a group's values, in order; the switch is taken once
__device__ inline uint32_t accumulateGroup(uint32_t kind, uint32_t acc,
                                           const uint32_t (&x)[kReduceGroup], uint32_t n)
{
#define REDUCE_GROUP_CASE(K) \
    case K: \
        _Pragma("unroll") \
        for (uint32_t i = 0; i < kReduceGroup; i++) { \
            if (i < n) acc = accumulate(K, acc, x[i]); \
        } \
        return acc;
    switch (kind & kKindMask) {
    REDUCE_GROUP_CASE(kSumF)
    REDUCE_GROUP_CASE(kSumI)
    REDUCE_GROUP_CASE(kMinF)
    REDUCE_GROUP_CASE(kMinI)
    REDUCE_GROUP_CASE(kMinU)
    REDUCE_GROUP_CASE(kMaxF)
    REDUCE_GROUP_CASE(kMaxI)
    REDUCE_GROUP_CASE(kMaxU)
    REDUCE_GROUP_CASE(kAbsMax)
    REDUCE_GROUP_CASE(kNonZeroF)
    REDUCE_GROUP_CASE(kNonZeroI)
    REDUCE_GROUP_CASE(kNonFinite)
    default: return acc;
    }
#undef REDUCE_GROUP_CASE
}

// row r into every accumulator of the lane
__device__ inline void reduceRow(ReduceSlot (&slots)[kReduceSlots], uint32_t num_slots, int32_t r)
{
#pragma unroll
    for (uint32_t k = 0; k < kReduceSlots; k++) {
        if (k < num_slots && slots[k].kind != kNone) {
            slots[k].acc = accumulate(slots[k].kind, slots[k].acc, loadElem(slots[k], r));
        }
    }
}

// rows [from, to), every one of them the world's: the loads of a group of rows
// in flight together (those past `to` read row to - 1 again and are not
// accumulated), then the accumulations in row order
__device__ inline void reduceRange(ReduceSlot (&slots)[kReduceSlots], uint32_t num_slots,
                                   int32_t from, int32_t to)
{
    for (int32_t r = from; r < to; r += (int32_t)kReduceGroup) {
        const uint32_t n = (uint32_t)(to - r) < kReduceGroup ? (uint32_t)(to - r) : kReduceGroup;
#pragma unroll
        for (uint32_t k = 0; k < kReduceSlots; k++) {
            if (k < num_slots && slots[k].kind != kNone) {
                uint32_t x[kReduceGroup];
#pragma unroll
                for (uint32_t i = 0; i < kReduceGroup; i++) {
                    x[i] = loadElem(slots[k], i < n ? r + (int32_t)i : to - 1);
                }
                slots[k].acc = accumulateGroup(slots[k].kind, slots[k].acc, x, n);
            }
        }
    }
}

// Rows [from, to) of the table, T at a time: those whose WorldID cell is w go
// into the accumulators, lowest row first.  from, to and w are the same in
// every lane of a team.  Returns the rows found.
__device__ inline uint32_t reduceRows(ReduceSlot (&slots)[kReduceSlots], uint32_t num_slots,
                                      const int32_t *world_col, int32_t from, int32_t to,
                                      uint32_t w, uint32_t t, uint32_t T, uint32_t team_shift,
                                      unsigned long long team_bits)
{
    uint32_t found = 0;
    for (int32_t base = from; base < to; base += (int32_t)T) {
        const int32_t r = base + (int32_t)t;
        const bool is = r < to && world_col[r] == (int32_t)w;
        unsigned long long m = (__ballot(is) >> team_shift) & team_bits;
        found += (uint32_t)__builtin_popcountll(m);
        while (m != 0ull) {
            const int32_t bit = (int32_t)__builtin_ctzll(m);
            m &= m - 1ull;
            reduceRow(slots, num_slots, base + bit);
        }
    }
    return found;
}

// one wavefront, 64 / T consecutive worlds of one reduce
__device__ inline void reduceWave(const ReducePlan *plan, uint32_t item, uint32_t lane)
{
    const uint32_t T = plan->teamLanes;
    const uint32_t num_worlds = plan->numWorlds;
    const uint32_t num_elems = plan->numElems;
    const uint32_t num_slots = (num_elems + 63u) / 64u;     // (more than one: T == 64)
    const uint32_t team = lane / T;
    const uint32_t t = lane & (T - 1u);
    const uint32_t team_shift = team * T;
    const unsigned long long team_bits = T >= 64u ? ~0ull : (1ull << T) - 1ull;
    const uint32_t w = item * (64u / T) + team;
    const bool valid = w < num_worlds;

    const madrona::mwhip::TeamRange range = madrona::mwhip::teamRange(plan->hdr, w, valid);
    const int32_t n = range.n, prefix = range.prefix, lo = range.lo, hi = range.hi;
    const int32_t *world_col = range.worldCol;

    // the lane's elements
    ReduceSlot slots[kReduceSlots];
#pragma unroll
    for (uint32_t k = 0; k < kReduceSlots; k++) {
        slots[k].src = nullptr;
        slots[k].stride = 0u;
        slots[k].kind = kNone;
        slots[k].acc = 0u;
        const uint32_t e = t + k * 64u;
        if (k < num_slots && e < num_elems && valid) {
            const ReducePlanElem &elem = plan->elems[e];
            slots[k].src = (const char *)*elem.slot + elem.byteOffset;
            slots[k].stride = elem.cellBytes;
            slots[k].kind = elem.kind;
            slots[k].acc = elem.identity;
        }
    }

    // 1. the live rows of the range
    uint32_t live = 0;
    for (int32_t base = lo; base < hi; base += (int32_t)T) {
        const int32_t r = base + (int32_t)t;
        const bool is = r < hi && world_col[r] == (int32_t)w;
        live += (uint32_t)__builtin_popcountll((__ballot(is) >> team_shift) & team_bits);
    }

    // 2. walk them
    if (live == (uint32_t)(hi - lo)) {
        reduceRange(slots, num_slots, lo, hi);
    } else {
        (void)reduceRows(slots, num_slots, world_col, lo, hi, w, t, T, team_shift, team_bits);
    }

    // 3. the rows behind the prefix (decided here, per table, from the header)
    uint32_t count = live;
    if (valid) {
        count += reduceRows(slots, num_slots, world_col, prefix, n, w, t, T, team_shift,
                            team_bits);
    }

    // 4. results, count and alarm
    bool trip = false;
#pragma unroll
    for (uint32_t k = 0; k < kReduceSlots; k++) {
        const uint32_t e = t + k * 64u;
        if (k < num_slots && slots[k].kind != kNone) {
            const ReducePlanElem &elem = plan->elems[e];
            const uint32_t acc = slots[k].acc;
            ((GlobalU32 *)(uint64_t)elem.out)[(uint64_t)w * elem.outStride] = acc;
            if (elem.alarm != 0u) {
                const uint32_t kind = slots[k].kind & kKindMask;
                if (kind == kMinF) {
                    trip = trip || __uint_as_float(acc) < elem.limit;
                } else if (kind == kMaxF || kind == kAbsMax) {
                    trip = trip || __uint_as_float(acc) > elem.limit;
                } else {
                    trip = trip || (int32_t)acc > 0;
                }
            }
        }
    }
    const unsigned long long tripped = (__ballot(trip) >> team_shift) & team_bits;
    if (valid && t == 0u) {
        plan->counts[w] = (int32_t)count;
        plan->alarm[w] = tripped != 0ull ? 1 : 0;
    }
}

__global__ void __launch_bounds__(kReduceThreads)
worldReduceKernel(ReduceArgs args)
{
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t total = 0;
#pragma unroll
    for (uint32_t v = 0; v < MWHIP_MAX_STEP_REDUCES; v++) {
        if (v < args.num_plans) total += args.items[v];
    }
    for (uint32_t item = blockIdx.x * kReduceWaves + wave; item < total;
         item += gridDim.x * kReduceWaves) {
        // the reduce this item belongs to (constant indices: the arguments stay
        // in scalar registers)
        const ReducePlan *plan = nullptr;
        uint32_t rel = item;
#pragma unroll
        for (uint32_t v = 0; v < MWHIP_MAX_STEP_REDUCES; v++) {
            if (plan == nullptr && v < args.num_plans) {
                if (rel < args.items[v]) {
                    plan = args.plans[v];
                } else {
                    rel -= args.items[v];
                }
            }
        }
        if (plan != nullptr) {
            reduceWave(plan, rel, lane);
        }
    }
}

}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct mwhip_reduce_rec {
    uint64_t handle = 0;
    uint32_t numWorlds = 0;
    uint32_t items = 0;         // wavefront work items
    uint32_t numElems = 0;      // of all terms
    uint32_t rowBytes = 0;      // of the listed elements of one row
    std::vector<uint32_t> termElems;
    std::vector<char *> outs;   // into bufDev
    int32_t *countsDev = nullptr;
    int32_t *alarmDev = nullptr;
    ReducePlan *planDev = nullptr;
    char *bufDev = nullptr;     // the results (256-byte aligned each), counts, alarms

    ~mwhip_reduce_rec()
    {
        if (planDev != nullptr) (void)hipFree(planDev);
        if (bufDev != nullptr) (void)hipFree(bufDev);
    }
};

namespace {

mwhip_reduce_rec *findReduce(mwhip_exec *exec, uint64_t handle)
{
    return findObject(exec != nullptr ? &exec->reduces : nullptr, handle);
}

dim3 reduceGrid(mwhip_exec *exec, uint32_t items)
{
    return waveGrid(exec, items, kReduceWaves, 16u);
}

int queueReduce(mwhip_exec *exec, mwhip_reduce_rec &reduce)
{
    return queueBatch(exec, (const void *)&worldReduceKernel, reduceGrid(exec, reduce.items),
                      kReduceThreads, singleBatch<ReduceArgs>(reduce));
}

int computeReduce(mwhip_exec *exec, uint64_t handle, bool wait)
{
    return computeObject(exec, findReduce(exec, handle), "reduce", handle, wait, queueReduce);
}

// Bytes the step reduces' last run read: per row counted its WorldID cell and
// its listed elements (KernelLaunch::measuredBytes).
int stepReduceReadBytes(mwhip_exec *exec, double *out)
{
    *out = 0;
    std::vector<int32_t> counts;
    for (uint64_t handle : exec->extras.stepReduces) {
        mwhip_reduce_rec *reduce = findReduce(exec, handle);
        if (reduce == nullptr) continue;
        counts.resize(reduce->numWorlds);
        HIPCHK(hipMemcpy(counts.data(), reduce->countsDev, counts.size() * sizeof(int32_t),
                         hipMemcpyDeviceToHost));
        for (int32_t count : counts) {
            *out += (double)std::max(count, 0) * (4.0 + reduce->rowBytes);
        }
    }
    return 0;
}

uint32_t reduceElemBytes(uint32_t dtype)
{
    return dtype == MWHIP_REDUCE_U8 ? 1u : 4u;
}

// (op, dtype) -> what the accumulators do and start from; kNone: no such pair
uint32_t reduceKind(uint32_t op, uint32_t dtype, uint32_t *identity)
{
    const bool f = dtype == MWHIP_REDUCE_F32;
    const bool i = dtype == MWHIP_REDUCE_I32;
    const uint32_t load = dtype == MWHIP_REDUCE_U8 ? kLoadU8 : 0u;
    *identity = 0u;
    switch (op) {
    case MWHIP_REDUCE_SUM:
        return (f ? kSumF : kSumI) | load;
    case MWHIP_REDUCE_MIN:
        *identity = f ? 0x7F800000u : i ? 0x7FFFFFFFu : 0xFFFFFFFFu;
        return (f ? kMinF : i ? kMinI : kMinU) | load;
    case MWHIP_REDUCE_MAX:
        *identity = f ? 0xFF800000u : i ? 0x80000000u : 0u;
        return (f ? kMaxF : i ? kMaxI : kMaxU) | load;
    case MWHIP_REDUCE_ABSMAX:
        return f ? kAbsMax : kNone;
    case MWHIP_REDUCE_COUNT_NONZERO:
        return (f ? kNonZeroF : kNonZeroI) | load;
    case MWHIP_REDUCE_COUNT_NONFINITE:
        return f ? kNonFinite : kNone;
    default:
        return kNone;
    }
}

}

// Tail stage: the ONE launch that recomputes every step reduce inside a step
// replay; none when no step reduce is set.
MWHIP_RT int stepReduceStage(mwhip_exec *exec, const LaunchGraph &lg,
                             std::vector<KernelLaunch> &out)
{
    if (lg.isRender) return 0;
    ReduceArgs args {};
    double written = 0;
    const uint32_t items = collectStepBatch(
        exec->extras.stepReduces, exec->reduces, args, [&](const mwhip_reduce_rec &reduce) {
            written += (double)reduce.numWorlds * (4.0 * reduce.numElems + 8.0);
        });
    if (args.num_plans == 0) return 0;
    // (what the step reduces read: from the counts they just left)
    out.push_back(stageLaunch((const void *)&worldReduceKernel, reduceGrid(exec, items),
                              kReduceThreads, args, "reduce", "reduce", written,
                              &stepReduceReadBytes));
    return 0;
}

extern "C" int mwhip_reduce_create(mwhip_exec *exec, uint32_t archetype_id,
                                   const mwhip_reduce_term *terms, uint32_t n,
                                   uint64_t *reduce_out)
{
    carryStale(exec);
    // (every refusal comes before anything is allocated)
    if (exec == nullptr || !exec->stateBuilt || reduce_out == nullptr) {
        return fail(-2, "reduce_create: no executor state");
    }
    if (n == 0 || terms == nullptr) {
        return fail(-2, "reduce_create: no terms (n == 0)");
    }
    if (n > MWHIP_REDUCE_MAX_TERMS) {
        return fail(-2, "reduce_create: %u terms (at most %u)", n,
                    (uint32_t)MWHIP_REDUCE_MAX_TERMS);
    }
    std::vector<ReduceTermInfo> infos(n);
    std::vector<mwhip_digest_column> distinct;
    uint64_t num_elems = 0;
    for (uint32_t p = 0; p < n; p++) {
        const mwhip_reduce_term &term = terms[p];
        if (term.num_elems == 0) {
            return fail(-2, "reduce_create: term %u: num_elems == 0", p);
        }
        if (term.dtype > MWHIP_REDUCE_U8) {
            return fail(-2, "reduce_create: term %u: unknown dtype %u", p, term.dtype);
        }
        if (term.op > MWHIP_REDUCE_COUNT_NONFINITE) {
            return fail(-2, "reduce_create: term %u: unknown op %u", p, term.op);
        }
        if ((term.flags & ~(uint32_t)MWHIP_REDUCE_ALARM) != 0u) {
            return fail(-2, "reduce_create: term %u: unknown flags 0x%x", p, term.flags);
        }
        uint32_t identity = 0;
        const uint32_t kind = reduceKind(term.op, term.dtype, &identity);
        if (kind == kNone) {
            return fail(-2, "reduce_create: term %u: op %u needs F32 elements (dtype %u)", p,
                        term.op, term.dtype);
        }
        const bool alarm = (term.flags & MWHIP_REDUCE_ALARM) != 0u;
        const bool counts = term.op == MWHIP_REDUCE_COUNT_NONZERO ||
            term.op == MWHIP_REDUCE_COUNT_NONFINITE;
        const bool bounded = term.dtype == MWHIP_REDUCE_F32 &&
            (term.op == MWHIP_REDUCE_MIN || term.op == MWHIP_REDUCE_MAX ||
             term.op == MWHIP_REDUCE_ABSMAX);
        if (alarm && !counts && !bounded) {
            return fail(-2, "reduce_create: term %u: an alarm has no rule for op %u on dtype %u",
                        p, term.op, term.dtype);
        }
        const uint32_t elem_bytes = reduceElemBytes(term.dtype);
        if (term.byte_offset % elem_bytes != 0u) {
            return fail(-2, "reduce_create: term %u: byte_offset %u is not a multiple of the "
                        "element size %u", p, term.byte_offset, elem_bytes);
        }
        num_elems += term.num_elems;
        if (num_elems > MWHIP_REDUCE_MAX_ELEMS) {
            return fail(-2, "reduce_create: more than %u elements in all (at most %u)",
                        (uint32_t)MWHIP_REDUCE_MAX_ELEMS, (uint32_t)MWHIP_REDUCE_MAX_ELEMS);
        }
        uint32_t c = 0;
        while (c < distinct.size() && distinct[c].component_id != term.component_id) c++;
        if (c == distinct.size()) distinct.push_back({ archetype_id, term.component_id });
        ReduceTermInfo &pt = infos[p];
        pt.column = c;
        pt.byteOffset = term.byte_offset;
        pt.numElems = term.num_elems;
        pt.firstElem = (uint32_t)(num_elems - term.num_elems);
        pt.kind = kind;
        pt.elemBytes = elem_bytes;
        pt.alarm = alarm ? 1u : 0u;
        pt.identity = identity;
        pt.limit = term.limit;
    }
    std::vector<ResolvedColumn> columns;
    int rc = resolveColumns(exec, "reduce_create", distinct.data(), (uint32_t)distinct.size(),
                            columns);
    if (rc != 0) return rc;
    uint32_t row_bytes = 0;
    for (uint32_t p = 0; p < n; p++) {
        const ReduceTermInfo &pt = infos[p];
        const uint32_t cell = columns[pt.column].cellBytes;
        if (cell % pt.elemBytes != 0u) {
            return fail(-2, "reduce_create: term %u: cells of %u bytes are not a multiple of the "
                        "element size %u", p, cell, pt.elemBytes);
        }
        if ((uint64_t)pt.byteOffset + (uint64_t)pt.numElems * pt.elemBytes > cell) {
            return fail(-2, "reduce_create: term %u: %u elements of %u bytes at offset %u leaves "
                        "the cell (%u bytes)", p, pt.numElems, pt.elemBytes, pt.byteOffset, cell);
        }
        row_bytes += pt.numElems * pt.elemBytes;
    }

    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    std::unique_ptr<mwhip_reduce_rec> reduce(new mwhip_reduce_rec {});
    reduce->numWorlds = exec->cfg.num_worlds;
    reduce->numElems = (uint32_t)num_elems;
    reduce->rowBytes = row_bytes;
    uint32_t team = 1;
    while (team < 64u && team < reduce->numElems) team <<= 1;
    const uint32_t per_wave = 64u / team;
    reduce->items = (reduce->numWorlds + per_wave - 1u) / per_wave;

    // the results, 256-byte aligned each, then the counts and the alarms
    std::vector<uint64_t> offsets(n);
    uint64_t total = 0;
    for (uint32_t p = 0; p < n; p++) {
        reduce->termElems.push_back(infos[p].numElems);
        offsets[p] = total;
        const uint64_t bytes = (uint64_t)reduce->numWorlds * infos[p].numElems * 4ull;
        total += (bytes + 255ull) & ~255ull;
    }
    const uint64_t per_world = ((uint64_t)reduce->numWorlds * sizeof(int32_t) + 255ull) & ~255ull;
    const uint64_t counts_at = total;
    const uint64_t alarm_at = total + per_world;
    total += 2ull * per_world;

    bool ok = hipMalloc((void **)&reduce->bufDev, total) == hipSuccess &&
        hipMalloc((void **)&reduce->planDev, sizeof(ReducePlan)) == hipSuccess &&
        hipMemset(reduce->bufDev, 0, total) == hipSuccess;
    if (ok) {
        reduce->countsDev = (int32_t *)(reduce->bufDev + counts_at);
        reduce->alarmDev = (int32_t *)(reduce->bufDev + alarm_at);
        // (12 KiB: not on the stack)
        std::unique_ptr<ReducePlan> plan_host(new ReducePlan {});
        ReducePlan &plan = *plan_host;
        plan.hdr = exec->hostState.tables + archetype_id;   // (a device address: never read here)
        plan.counts = reduce->countsDev;
        plan.alarm = reduce->alarmDev;
        plan.numWorlds = reduce->numWorlds;
        plan.numElems = reduce->numElems;
        plan.numTerms = n;
        plan.teamLanes = team;
        for (uint32_t p = 0; p < n; p++) {
            reduce->outs.push_back(reduce->bufDev + offsets[p]);
            const ReduceTermInfo &pt = infos[p];
            for (uint32_t e = 0; e < pt.numElems; e++) {
                plan.elems[pt.firstElem + e] = {
                    columns[pt.column].slot, (uint32_t *)reduce->outs[p] + e,
                    pt.byteOffset + e * pt.elemBytes, columns[pt.column].cellBytes, pt.kind,
                    pt.identity, pt.numElems, pt.alarm, pt.limit, 0u };
            }
        }
        ok = hipMemcpy(reduce->planDev, &plan, sizeof(plan), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        return CREATE_FAILED(reduce, "reduce_create: no device memory for the plan and %llu "
                             "bytes (%u worlds x %u elements)", (unsigned long long)total,
                             exec->cfg.num_worlds, (uint32_t)num_elems);
    }
    *reduce_out = exec->reduces.insert(std::move(reduce));
    return 0;
}

extern "C" int mwhip_set_step_reduce(mwhip_exec *exec, uint64_t reduce, int on)
{
    carryStale(exec);
    if (findReduce(exec, reduce) == nullptr) return unknownObject("reduce", reduce);
    return toggleStepSet(exec, &ReplayExtras::stepReduces, reduce, on, MWHIP_MAX_STEP_REDUCES,
                         "set_step_reduce", "step reduces");
}

extern "C" void mwhip_reduce_destroy(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    destroyStepObject(exec, &mwhip_exec::reduces, handle, &mwhip_set_step_reduce);
}

extern "C" int mwhip_reduce_compute(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeReduce(exec, handle, true);
}

extern "C" int mwhip_reduce_compute_async(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeReduce(exec, handle, false);
}

extern "C" void *mwhip_reduce_buffer(mwhip_exec *exec, uint64_t handle, uint32_t term,
                                     uint64_t *bytes_out, uint32_t *elems_out)
{
    mwhip_reduce_rec *reduce = findReduce(exec, handle);
    if (reduce == nullptr) {
        (void)unknownObject("reduce", handle);
        return nullptr;
    }
    if (term >= reduce->outs.size()) {
        (void)fail(-2, "reduce_buffer: term %u of %u", term, (uint32_t)reduce->outs.size());
        return nullptr;
    }
    if (bytes_out != nullptr) {
        *bytes_out = (uint64_t)reduce->numWorlds * reduce->termElems[term] * 4ull;
    }
    if (elems_out != nullptr) *elems_out = reduce->termElems[term];
    return reduce->outs[term];
}

extern "C" int32_t *mwhip_reduce_counts(mwhip_exec *exec, uint64_t handle)
{
    mwhip_reduce_rec *reduce = findReduce(exec, handle);
    if (reduce == nullptr) {
        (void)unknownObject("reduce", handle);
        return nullptr;
    }
    return reduce->countsDev;
}

extern "C" int32_t *mwhip_reduce_alarm(mwhip_exec *exec, uint64_t handle)
{
    mwhip_reduce_rec *reduce = findReduce(exec, handle);
    if (reduce == nullptr) {
        (void)unknownObject("reduce", handle);
        return nullptr;
    }
    return reduce->alarmDev;
}
