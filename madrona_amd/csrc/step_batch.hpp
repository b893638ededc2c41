// Step-batched executor objects: what world views, world writes, world reduces,
// entity gathers, entity scatters, ray queries, box queries, contact queries and shape
// queries share on the host beyond exec_objects.hpp.  Such an object can be computed (or
// applied) alone, or be SET: every step replay then serves all set objects of
// its kind in ONE launch whose argument is a batch of their plans
// (madrona/mwhip/plan_batch.hpp).  Here, once: the step set and its cap, the
// destroy of an object that may be set, the batch of one and of the set, the
// launch that carries a batch, its grid.  Host code only.  Not a header to
// include on its own: exec_internal.hpp includes it at its end, behind
// mwhip_exec, ReplayExtras and changeReplayExtras.  Not installed.
#pragma once
#include <madrona/mwhip/plan_batch.hpp>

#include <algorithm>

// mwhip_set_step_<kind>, behind the entry point's lookup of the object: puts
// `handle` into the step set `set` or takes it out and rebuilds the launch
// graphs; nothing when it is where it should be already.  At most `cap` are
// set: -2, "<entry>: N <plural> are set already (at most cap)".  `admit` may
// refuse (non-zero) an object that is about to be set, behind the cap.
template <typename Admit>
inline int toggleStepSet(mwhip_exec *exec, std::vector<uint64_t> ReplayExtras::*set,
                         uint64_t handle, int on, uint32_t cap, const char *entry,
                         const char *plural, Admit &&admit)
{
    const std::vector<uint64_t> &now = exec->extras.*set;
    const bool is_on = std::find(now.begin(), now.end(), handle) != now.end();
    if (is_on == (on != 0)) return 0;
    if (on != 0) {
        if (now.size() >= cap) {
            return fail(-2, "%s: %u %s are set already (at most %u)", entry, (uint32_t)now.size(),
                        plural, cap);
        }
        const int rc = admit();
        if (rc != 0) return rc;
    }
    return changeReplayExtras(exec, [set, handle, on](ReplayExtras &extras) {
        std::vector<uint64_t> &handles = extras.*set;
        if (on != 0) {
            handles.push_back(handle);
        } else {
            handles.erase(std::find(handles.begin(), handles.end(), handle));
        }
        return 0;
    });
}

inline int toggleStepSet(mwhip_exec *exec, std::vector<uint64_t> ReplayExtras::*set,
                         uint64_t handle, int on, uint32_t cap, const char *entry,
                         const char *plural)
{
    return toggleStepSet(exec, set, handle, on, cap, entry, plural, [] { return 0; });
}

// mwhip_<kind>_destroy, behind carryStale: `unset` is the kind's own
// mwhip_set_step_<kind>.  The step graphs must stop naming the object's buffers
// before they go; if they could not be rebuilt without it, it stays allocated
// and in its table until mwhip_destroy.
template <typename Rec>
inline void destroyStepObject(mwhip_exec *exec, ExecObjectTable<Rec> mwhip_exec::*table,
                              uint64_t handle, int (*unset)(mwhip_exec *, uint64_t, int))
{
    if (exec == nullptr || (exec->*table).find(handle) == nullptr) return;
    (void)hipSetDevice(exec->cfg.gpu_id);
    if (unset(exec, handle, 0) != 0) return;
    (void)hipStreamSynchronize(exec->stream);
    (exec->*table).erase(handle);
}

// Wavefronts stride over `items` work items, waves_per_block of them to a
// workgroup: as many workgroups as that takes, at most blocks_per_cu per CU, at
// least one.
inline dim3 waveGrid(const mwhip_exec *exec, uint32_t items, uint32_t waves_per_block,
                     uint32_t blocks_per_cu)
{
    const uint32_t blocks = (items + waves_per_block - 1u) / waves_per_block;
    return dim3(std::max(std::min(blocks, std::max(exec->numCUs, 1u) * blocks_per_cu), 1u), 1, 1);
}

// The batch of ONE object: what a compute or an apply launches with.  Args is a
// PlanBatch, mwhip_ray_args, mwhip_box_args, mwhip_contact_args or mwhip_shape_args; a record has
// items and planDev.
template <typename Args, typename Rec>
inline Args singleBatch(const Rec &rec)
{
    Args args {};
    args.num_plans = 1;
    args.items[0] = rec.items;
    args.plans[0] = rec.planDev;
    return args;
}

// The batch of a step set: the objects `set` names that `table` still has, as
// many as the batch holds (the set's cap), in the order they were set.
// per_rec(rec) sees each one taken (a kind sums its bytes there).  Returns the
// work items of all of them; args.num_plans == 0: nothing to launch.
template <typename Args, typename Rec, typename PerRec>
inline uint32_t collectStepBatch(const std::vector<uint64_t> &set,
                                 const ExecObjectTable<Rec> &table, Args &args,
                                 PerRec &&per_rec)
{
    constexpr uint32_t cap = sizeof(args.items) / sizeof(args.items[0]);
    uint32_t items = 0;
    for (uint64_t handle : set) {
        Rec *rec = table.find(handle);
        if (rec == nullptr || args.num_plans >= cap) continue;
        args.items[args.num_plans] = rec->items;
        args.plans[args.num_plans] = rec->planDev;
        args.num_plans += 1;
        items += rec->items;
        per_rec(*rec);
    }
    return items;
}

// A compute or an apply: `fn(args)` on the executor's stream.  (What the launch
// itself returns is checked; a sticky error an earlier call left is not looked
// for here, nor cleared: the next synchronize reports it.)
template <typename Args>
inline int queueBatch(mwhip_exec *exec, const void *fn, dim3 grid, uint32_t threads,
                      const Args &args)
{
    void *argv[] = { (void *)&args };
    HIPCHK(hipLaunchKernel(fn, grid, dim3(threads), argv, 0, exec->stream));
    return 0;
}

// The same launch as a stage of a step replay (TailStage, runtime_launch.hip).
template <typename Args>
inline KernelLaunch stageLaunch(const void *fn, dim3 grid, uint32_t threads, const Args &args,
                                const char *name, const char *role, double fixed_bytes,
                                int (*measured_bytes)(mwhip_exec *, double *) = nullptr)
{
    KernelLaunch k;
    static_assert(sizeof(Args) <= sizeof(k.argStorage));
    k.fn = fn;
    k.grid = grid;
    k.block = dim3(threads, 1, 1);
    k.setArgs(args);
    k.name = name;
    k.role = role;
    k.kind = MWHIP_NODE_RECYCLE;
    k.fixedBytes = fixed_bytes;
    k.measuredBytes = measured_bytes;
    return k;
}

// mwhip_<kind>_compute / _apply and their _async forms, behind carryStale:
// `rec` is what the entry point's lookup found (null: -3), queue(exec, rec)
// launches.
template <typename Rec, typename Queue>
inline int computeObject(mwhip_exec *exec, Rec *rec, const char *kind, uint64_t handle,
                         bool wait, Queue &&queue)
{
    if (rec == nullptr) return unknownObject(kind, handle);
    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    return finishQueued(exec, queue(exec, *rec), wait);
}
