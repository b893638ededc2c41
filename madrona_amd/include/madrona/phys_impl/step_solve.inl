// Part of the fused rigid-body step (phys_impl/step_lds.inl includes it in front
// of its kernel, inside namespace madrona::phys::kernels): the constraint solve
// of one substep over a world resident in LDS -- what physicsStepLdsKernel runs
// between its narrowphase and the next substep, in a function of its own so
// that the function-level solver tests (tests/shims/phys_device_shim.hip) call
// the kernel's code and not a copy of it.

// Position solve (the contact windows, then the joints), velocities from the
// poses, velocity solve: level by level, two lanes per constraint.
// lane: index inside the world's group of LPW lanes; every lane of the group is
// in the call.  joints: the world's rows in the sorted joint table (read for
// joints beyond Block::maxJoints).  prof(slot): the caller's phase-profile mark.
template <int MAXB, int LPW, typename ProfT>
__device__ __forceinline__ void solveSubstepConstraints(
    const uint32_t lane, WorldBlock<MAXB, LPW> *w,
    LdsBodyStore<MAXB, LPW> &store, const int32_t num_bodies,
    const uint32_t num_contacts, const int32_t num_joints,
    const JointConstraint *joints, ProfT &&prof)
{
    using Block = WorldBlock<MAXB, LPW>;

    // ---- position solve: contacts, then joints, level by level ----------
    // (the levels of the first window of contacts -- all of them, in
    // every world seen so far -- serve the velocity solve as well: same
    // contacts, same bodies)
    uint32_t first_level = 0, first_max_level = 0;
    for (uint32_t base = 0; base < num_contacts; base += LPW) {
        const uint32_t n = num_contacts - base < (uint32_t)LPW ?
            num_contacts - base : (uint32_t)LPW;
        const uint32_t i = base + lane;
        uint32_t key_a = 0, key_b = 0;
        if (lane < n) {
            key_a = ldsBodyKey(w, w->contacts()[i].refBody());
            key_b = ldsBodyKey(w, w->contacts()[i].altBody());
        }
        uint32_t level = constraintLevels<LPW>(lane, n, key_a, key_b);
        uint32_t max_level = wave::maxReduce<LPW>(lane < n ? level : 0);
        if (base == 0) {
            first_level = level;
            first_max_level = max_level;
        }

        for (uint32_t l = 0; l <= max_level; l++) {
            // two lanes per contact, a body each (xpbd::paired): the
            // level's contacts in index order over the world's teams
            const uint64_t members =
                wave::groupBallot<LPW>(lane < n && level == l);
            const uint32_t count = (uint32_t)__builtin_popcountll(members);
            for (uint32_t first = 0; first < count; first += LPW / 2) {
                const uint32_t team = first + (lane >> 1);
                if (team < count) {
                    const uint32_t ci =
                        base + wave::nthSetBit<LPW>(members, team);
                    const bool second = (lane & 1u) != 0u;
                    float lambda_n[4] { 0.f, 0.f, 0.f, 0.f };
                    xpbd::paired::handleContact(second, store,
                        w->contacts()[ci].view(), lambda_n);
                    if (!second) {
                        w->lambdas[ci] = lambda_n[0];
                    }
                }
            }
            wave::phaseFence();
        }
    }

    // (at most maxJointBodies of them: one window)
    if (num_joints > 0) {
        const uint32_t n = (uint32_t)num_joints;
        Loc l1 { 0, 0 }, l2 { 0, 0 };
        uint32_t key_a = 0, key_b = 0;
        if (lane < n) {
            l1 = Loc { 0, (int32_t)w->jointBodies[lane][0] };
            l2 = Loc { 0, (int32_t)w->jointBodies[lane][1] };
            key_a = ldsBodyKey(w, l1.row);
            key_b = ldsBodyKey(w, l2.row);
        }
        uint32_t level = constraintLevels<LPW>(lane, n, key_a, key_b);
        uint32_t max_level = wave::maxReduce<LPW>(lane < n ? level : 0);

        for (uint32_t l = 0; l <= max_level; l++) {
            // (two lanes per joint, an end each; at most maxJointBodies
            // joints: one round of teams)
            const uint64_t members =
                wave::groupBallot<LPW>(lane < n && level == l);
            const uint32_t team = lane >> 1;
            if (team < (uint32_t)__builtin_popcountll(members)) {
                const uint32_t j = wave::nthSetBit<LPW>(members, team);
                const bool second = (lane & 1u) != 0u;
                const Loc me { 0, (int32_t)w->jointBodies[j][second ? 1 : 0] };
                // (rows beyond the block's: out of the sorted table)
                xpbd::paired::handleJointConstraint(second, store, me,
                    j < (uint32_t)Block::maxJoints ? w->joints[j] : joints[j]);
            }
            wave::phaseFence();
        }
    }

    prof(4);
    // ---- velocities -----------------------------------------------------
    for (int32_t k = (int32_t)lane; k < num_bodies; k += LPW) {
        w->vel[k] = xpbd::deriveVelocity(w->poses[k].x, w->poses[k].q,
            store.prevState(Loc { 0, k }), w->sys.h);
    }
    wave::phaseFence();
    prof(4);

    for (uint32_t base = 0; base < num_contacts; base += LPW) {
        const uint32_t n = num_contacts - base < (uint32_t)LPW ?
            num_contacts - base : (uint32_t)LPW;
        const uint32_t i = base + lane;
        uint32_t level = first_level;
        uint32_t max_level = first_max_level;
        if (base != 0) {
            uint32_t key_a = 0, key_b = 0;
            if (lane < n) {
                key_a = ldsBodyKey(w, w->contacts()[i].refBody());
                key_b = ldsBodyKey(w, w->contacts()[i].altBody());
            }
            level = constraintLevels<LPW>(lane, n, key_a, key_b);
            max_level = wave::maxReduce<LPW>(lane < n ? level : 0);
        }

        for (uint32_t l = 0; l <= max_level; l++) {
            const uint64_t members =
                wave::groupBallot<LPW>(lane < n && level == l);
            const uint32_t count = (uint32_t)__builtin_popcountll(members);
            for (uint32_t first = 0; first < count; first += LPW / 2) {
                const uint32_t team = first + (lane >> 1);
                if (team < count) {
                    const uint32_t ci =
                        base + wave::nthSetBit<LPW>(members, team);
                    float lambda_n[4] { w->lambdas[ci], 0.f, 0.f, 0.f };
                    xpbd::paired::solveVelocitiesForContact(
                        (lane & 1u) != 0u, store,
                        w->contacts()[ci].view(), lambda_n, w->sys.h,
                        w->sys.restitutionThreshold);
                }
            }
            wave::phaseFence();
        }
    }
}
