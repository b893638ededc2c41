// libmadrona_hip.so -- contact queries: per world the primitive pairs of its
// rigid bodies that touch, with the manifold the step's narrowphase builds for
// each (mwhip_contacts_*, include/mwhip.h; DESIGN.md §36;
// madrona_amd/contact_ref.py is the definition).
//
// This file is the host side only, a sibling of box_query.hip.  The kernel,
// contactQueryKernel, is compiled into the simulator's code object
// (include/madrona/phys_impl/contact_query.inl), where the narrowphase lives;
// PhysicsSystem::setupPhysicsStepTasks registers its host stub
// (mwhip_set_contact_kernel) and the runtime launches it.  What the two code
// objects share is the POD pair mwhip_contact_plan / mwhip_contact_args of
// mwhip.h.  A query owns a device-resident plan and ONE allocation with its
// select buffer (if it owns one) and its outputs (status, count, pairs,
// num_points, normal, points), 256-byte aligned each.  A select source is read
// on the device when the kernel runs, as a ray query's sources.
#include "tree_query.hpp"

namespace {

constexpr uint32_t kContactThreads = 256;
constexpr uint32_t kContactWaves = kContactThreads / 64u;

}

struct mwhip_contacts_rec : TreeQueryRec<mwhip_contact_plan, MWHIP_CONTACTS_NUM_BUFS> {
    uint32_t numWorlds = 0;
    uint32_t maxContacts = 0;
    bool readsSelect = false;
};

namespace {

mwhip_contacts_rec *findContacts(mwhip_exec *exec, uint64_t handle)
{
    return findObject(exec != nullptr ? &exec->contacts : nullptr, handle);
}

// (a work item is a WORLD, whatever the number of plans: a wavefront serves its
// world for one plan after the other, so that no two wavefronts of a launch
// hold the same world's PhysicsScratch::worldHullScratch slot.  The cap of 8
// workgroups per CU is the ray kernel's -- registers hold this kernel to one
// wavefront per SIMD, one workgroup per CU at a time: DESIGN.md §36.)
dim3 contactGrid(mwhip_exec *exec, uint32_t worlds)
{
    return waveGrid(exec, worlds, kContactWaves, 8u);
}

int queueContacts(mwhip_exec *exec, mwhip_contacts_rec &contacts)
{
    return queueBatch(exec, exec->contactKernel, contactGrid(exec, contacts.numWorlds),
                      kContactThreads, singleBatch<mwhip_contact_args>(contacts));
}

int computeContacts(mwhip_exec *exec, uint64_t handle, bool wait)
{
    return computeObject(exec, findContacts(exec, handle), "contact query", handle, wait,
                         queueContacts);
}

}

// Tail stage: the ONE launch that recomputes every step contact query inside a
// step replay, directly behind the step box queries and in front of the step
// gathers (which may read the pairs); none when no step query is set.  It reads
// the tables and writes only the queries' own buffers, so it has no say in
// whether a steady replay drops its carried launches.
MWHIP_RT int stepContactsStage(mwhip_exec *exec, const LaunchGraph &lg,
                               std::vector<KernelLaunch> &out)
{
    if (lg.isRender || exec->contactKernel == nullptr) return 0;
    mwhip_contact_args args {};
    double bytes = 0;
    uint32_t worlds = 0;
    (void)collectStepBatch(
        exec->extras.stepContacts, exec->contacts, args, [&](const mwhip_contacts_rec &contacts) {
            // written: status, count and every contact slot (16 + 4 + 12 + 64
            // bytes); read: select.  The bodies' bytes depend on what touches
            // and are not counted.
            bytes += (double)contacts.numWorlds *
                (8.0 + 96.0 * (double)contacts.maxContacts + (contacts.readsSelect ? 4.0 : 0.0));
            worlds = contacts.numWorlds;
        });
    if (args.num_plans == 0) return 0;
    out.push_back(stageLaunch(exec->contactKernel, contactGrid(exec, worlds), kContactThreads,
                              args, "contacts", "contacts", bytes));
    return 0;
}

extern "C" int mwhip_set_contact_kernel(mwhip_exec *exec, const void *kernel, uint32_t caps)
{
    carryStale(exec);
    if (exec == nullptr) return fail(-2, "set_contact_kernel: no executor");
    if (kernel != nullptr) {
        exec->contactKernel = kernel;
        exec->contactCaps = caps;
    }
    return 0;
}

extern "C" int mwhip_contacts_create(mwhip_exec *exec, const mwhip_contacts_desc *desc,
                                     uint64_t *contacts_out)
{
    carryStale(exec);
    // (every refusal comes before anything is allocated)
    if (exec == nullptr || !exec->stateBuilt || contacts_out == nullptr) {
        return fail(-2, "contacts_create: no executor state");
    }
    if (desc == nullptr) return fail(-2, "contacts_create: no descriptor");
    if (exec->contactKernel == nullptr) {
        return fail(-2, "contacts_create: this simulator registered no contact kernel (it sets "
                    "up no rigid-body step: PhysicsSystem::setupPhysicsStepTasks)");
    }
    if ((desc->flags & ~(MWHIP_CONTACTS_CURRENT_POSES | MWHIP_CONTACTS_PLAIN)) != 0u) {
        return fail(-2, "contacts_create: unknown flags 0x%x", desc->flags);
    }
    if ((desc->flags & MWHIP_CONTACTS_CURRENT_POSES) == 0u &&
            (exec->contactCaps & MWHIP_CONTACT_CAP_SOLVER_POSES) == 0u) {
        return fail(-2, "contacts_create: this simulator has no solver poses (its solver keeps "
                    "no xpbd::PreSolvePositional): ask for MWHIP_CONTACTS_CURRENT_POSES");
    }
    if (desc->max_contacts == 0u) return fail(-2, "contacts_create: max_contacts is 0");
    const uint32_t W = exec->cfg.num_worlds, K = desc->max_contacts;
    if ((uint64_t)W * K * 2ull > 0x7FFFFFFFull) {
        return fail(-2, "contacts_create: %u worlds x %u contacts x 2 is more than %u handles", W,
                    K, 0x7FFFFFFFu);
    }
    const bool own_select = desc->own_select != 0u;
    if (desc->select.src != nullptr) {
        if (own_select) {
            return fail(-2, "contacts_create: select: a source and own_select were both given");
        }
        const int rc = checkItemSource("contacts_create", "select", desc->select, 4u);
        if (rc != 0) return rc;
    }

    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    std::unique_ptr<mwhip_contacts_rec> contacts(new mwhip_contacts_rec());
    contacts->numWorlds = W;
    contacts->maxContacts = K;
    contacts->readsSelect = own_select || desc->select.src != nullptr;
    contacts->items = W;

    const uint64_t slots = (uint64_t)W * K;
    contacts->bytes[MWHIP_CONTACTS_BUF_SELECT] = own_select ? (uint64_t)W * 4ull : 0ull;
    contacts->bytes[MWHIP_CONTACTS_BUF_STATUS] = (uint64_t)W * 4ull;
    contacts->bytes[MWHIP_CONTACTS_BUF_COUNT] = (uint64_t)W * 4ull;
    contacts->bytes[MWHIP_CONTACTS_BUF_PAIRS] = slots * 16ull;
    contacts->bytes[MWHIP_CONTACTS_BUF_NUM_POINTS] = slots * 4ull;
    contacts->bytes[MWHIP_CONTACTS_BUF_NORMAL] = slots * 12ull;
    contacts->bytes[MWHIP_CONTACTS_BUF_POINTS] = slots * 64ull;
    uint64_t total = 0;
    bool ok = allocQueryBuffers(*contacts, &total);
    if (ok) {
        // the outputs as a compute leaves a query whose worlds hold no contact
        ok = hipMemset(contacts->bufs[MWHIP_CONTACTS_BUF_PAIRS], 0xFF,
                       contacts->bytes[MWHIP_CONTACTS_BUF_PAIRS]) == hipSuccess;
    }
    if (ok && own_select) {
        // every world selected
        const std::vector<int32_t> ones(W, 1);
        ok = hipMemcpy(contacts->bufs[MWHIP_CONTACTS_BUF_SELECT], ones.data(), (size_t)W * 4u,
                       hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) {
        mwhip_contact_plan plan {};
        plan.state = exec->stateDev;
        resolveItemSource(own_select, contacts->bufs[MWHIP_CONTACTS_BUF_SELECT], 4u, desc->select,
                          &plan.select_src, &plan.select_stride);
        plan.status = (int32_t *)contacts->bufs[MWHIP_CONTACTS_BUF_STATUS];
        plan.count = (int32_t *)contacts->bufs[MWHIP_CONTACTS_BUF_COUNT];
        plan.pairs = (uint32_t *)contacts->bufs[MWHIP_CONTACTS_BUF_PAIRS];
        plan.num_points = (int32_t *)contacts->bufs[MWHIP_CONTACTS_BUF_NUM_POINTS];
        plan.normal = (float *)contacts->bufs[MWHIP_CONTACTS_BUF_NORMAL];
        plan.points = (float *)contacts->bufs[MWHIP_CONTACTS_BUF_POINTS];
        plan.max_contacts = K;
        plan.flags = desc->flags;
        plan.num_worlds = W;
        ok = hipMemcpy(contacts->planDev, &plan, sizeof(plan), hipMemcpyHostToDevice) ==
            hipSuccess;
    }
    if (!ok) {
        return CREATE_FAILED(contacts, "contacts_create: no device memory for the plan and %llu "
                             "bytes (%u worlds, %u contacts each)", (unsigned long long)total, W,
                             K);
    }
    *contacts_out = exec->contacts.insert(std::move(contacts));
    return 0;
}

extern "C" int mwhip_set_step_contacts(mwhip_exec *exec, uint64_t contacts, int on)
{
    carryStale(exec);
    if (findContacts(exec, contacts) == nullptr) return unknownObject("contact query", contacts);
    return toggleStepSet(exec, &ReplayExtras::stepContacts, contacts, on,
                         MWHIP_MAX_STEP_CONTACTS, "set_step_contacts", "step contact queries");
}

extern "C" void mwhip_contacts_destroy(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    destroyStepObject(exec, &mwhip_exec::contacts, handle, &mwhip_set_step_contacts);
}

extern "C" int mwhip_contacts_compute(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeContacts(exec, handle, true);
}

extern "C" int mwhip_contacts_compute_async(mwhip_exec *exec, uint64_t handle)
{
    carryStale(exec);
    return computeContacts(exec, handle, false);
}

extern "C" void *mwhip_contacts_buffer(mwhip_exec *exec, uint64_t handle, uint32_t which,
                                       uint64_t *bytes_out)
{
    return queryBuffer(findContacts(exec, handle), "contact query", handle, "contacts_buffer",
                       "no own_select", which, bytes_out);
}
