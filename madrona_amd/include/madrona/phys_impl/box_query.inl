// Box queries (mwhip_boxes_*, include/mwhip.h): tensors of
// boxes tested through the worlds' broadphase BVHs, the whole list of the
// entities PhysicsSystem::findEntitiesWithinAABB reports for each, in the order
// it reports them.  Included by physics.inl inside madrona::phys::kernels next
// to ray_query.inl, so the kernel is part of every simulator library that has a
// broadphase; PhysicsSystem::setupBroadphaseTasks hands the host stub to the
// runtime (mwhip_set_box_kernel), which owns the plans and launches it.
//
// One launch serves up to MWHIP_MAX_STEP_BOXES queries.  A workgroup is 256
// threads = 4 wavefronts = 8 groups of 32 lanes, no LDS.  A work item is a
// wavefront of ONE query; wavefronts stride over the items.
//   chunks_per_bundle > 0 (cooperative): group g of the query holds boxes
//       (g % chunks_per_bundle) * 32 + [0, 32) of bundle g / chunks_per_bundle.
//       Lane i of the group builds and checks box i of the chunk and every lane
//       takes all of them with cross-lane reads.  Then the group enumerates the
//       leaves of the world's tree in traversal order, 32 per window: lane i
//       tests the i-th leaf's own box against the chunk's boxes and runs the
//       hull test for those it meets (checkEntityAABBsOverlap<32>: the half
//       that does not depend on the box once).  Per box with a hit bit the
//       group's ballot ranks the accepting lanes: rank = the box's running
//       count + the accepting lanes below; lanes whose rank is below max_hits
//       store.  Report order is leaf order, which is findEntitiesWithinAABB's
//       (BVH::findIntersectingLeafBoxes).  While a rebuild of a built tree is
//       pending there is no such order: the group's first lane walks with
//       findEntitiesWithinAABB itself, box after box, as
//       findFirstEntitiesWithinAABBsWave does.
//   chunks_per_bundle == 0 (packed): box item * 64 + lane, whatever its bundle,
//       through plain findEntitiesWithinAABB with a callback that counts and
//       stores: the definition itself.
// Both leave the same words.  The two groups of a wavefront may hold different
// worlds, or one of them nothing: every ballot and every cross-lane read is cut
// to the group.  Checks come in the order world, count, centre (per bundle),
// then lo, hi, sums and pMin <= pMax (per box); nothing behind a failed check is
// read, and only a box whose status is OK goes to a tree, that of its (checked)
// world.  A world whose tree was never built (numNodes() == 0) gives count 0
// without the tree being touched.  Every store index is below its buffer's
// length: a box index is below B, a hit slot below max_hits.  No atomics, no
// spin-waits, no barrier, no workgroup waits for another; plain vector stores.

namespace boxq {

using treeq::finiteBits;

struct BundleHead {
    int32_t status;
    int32_t world;
    float cx, cy, cz;
};

// world, count and centre of bundle `bundle`, in that order, by ONE lane
__device__ inline BundleHead readBundle(const mwhip_box_plan *plan, const EcsState *S,
                                        uint32_t bundle)
{
    const treeq::GroupHead head = treeq::readGroupHead(
        plan->world_src, plan->world_stride, plan->count_src, plan->count_stride,
        plan->centre_src, plan->centre_stride, plan->bundles_per_world, bundle, S);
    const int32_t status = head.code == treeq::HeadCode::BadWorld ? MWHIP_BOXES_BAD_WORLD :
        head.code == treeq::HeadCode::Skipped ? MWHIP_BOXES_SKIPPED :
        head.code == treeq::HeadCode::BadPoint ? MWHIP_BOXES_BAD_BOX : MWHIP_BOXES_OK;
    return BundleHead { status, head.world, head.x, head.y, head.z };
}

// box `box` of a bundle whose head passed: OK or BAD_BOX
__device__ inline int32_t readBox(const mwhip_box_plan *plan, uint32_t box, float cx, float cy,
                                  float cz, math::AABB *out)
{
    const float *lo = plan->lo + (uint64_t)box * 3ull;
    const float *hi = plan->hi + (uint64_t)box * 3ull;
    const float l[3] { lo[0], lo[1], lo[2] };
    const float h[3] { hi[0], hi[1], hi[2] };
    const float c[3] { cx, cy, cz };
    float p_min[3], p_max[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        p_min[a] = c[a] + l[a];
        p_max[a] = c[a] + h[a];
        ok = ok && finiteBits(l[a]) && finiteBits(h[a]) && finiteBits(p_min[a]) &&
            finiteBits(p_max[a]) && p_min[a] <= p_max[a];
    }
    out->pMin = math::Vector3 { p_min[0], p_min[1], p_min[2] };
    out->pMax = math::Vector3 { p_max[0], p_max[1], p_max[2] };
    return ok ? MWHIP_BOXES_OK : MWHIP_BOXES_BAD_BOX;
}

__device__ inline void storeHit(const mwhip_box_plan *plan, uint32_t box, uint32_t slot,
                                Entity e)
{
    // (box < B, slot < max_hits: below B x max_hits <= 2^31 - 1)
    uint32_t *h = plan->hits + ((uint64_t)box * plan->max_hits + slot) * 2ull;
    h[0] = e.gen;
    h[1] = (uint32_t)e.id;
}

// one wavefront of a packed query: box item * 64 + lane
__device__ inline void boxWavePacked(const mwhip_box_plan *plan, uint32_t item, uint32_t lane)
{
    EcsState *S = (EcsState *)plan->state;
    StateManager *state_mgr = static_cast<StateManager *>(S);
    const uint32_t per_bundle = plan->boxes_per_bundle;
    const uint32_t max_hits = plan->max_hits;
    const uint64_t num_boxes = (uint64_t)plan->num_bundles * per_bundle;  // <= 2^31 - 1

    const uint64_t i = (uint64_t)item * 64ull + lane;
    if (i >= num_boxes) {
        return;
    }
    const uint32_t box = (uint32_t)i;
    const BundleHead head = readBundle(plan, S, box / per_bundle);
    int32_t status = head.status;
    math::AABB aabb {};
    if (status == MWHIP_BOXES_OK) {
        status = readBox(plan, box, head.cx, head.cy, head.cz, &aabb);
    }
    uint32_t count = 0;
    if (status == MWHIP_BOXES_OK) {
        Context ctx = TaskGraph::makeContext<Context>(state_mgr, WorldID { head.world });
        if (ctx.singleton<broadphase::BVH>().numNodes() != 0) {
            PhysicsSystem::findEntitiesWithinAABB(ctx, aabb, [&](Entity e) {
                if (count < max_hits) {
                    storeHit(plan, box, count, e);
                }
                count += 1u;
            });
        }
    }
    for (uint32_t k = count < max_hits ? count : max_hits; k < max_hits; k++) {
        storeHit(plan, box, k, Entity::none());
    }
    plan->status[box] = status;
    plan->count[box] = (int32_t)count;
}

// one wavefront of a cooperative query: groups 2 * item and 2 * item + 1
__device__ inline void boxWaveShared(const mwhip_box_plan *plan, uint32_t item, uint32_t lane)
{
    using broadphase::BVH;
    constexpr int32_t maxBoxes = 32;

    EcsState *S = (EcsState *)plan->state;
    StateManager *state_mgr = static_cast<StateManager *>(S);
    const uint32_t per_bundle = plan->boxes_per_bundle;
    const uint32_t max_hits = plan->max_hits;
    const uint32_t chunks = plan->chunks_per_bundle;

    const uint64_t group = (uint64_t)item * 2ull + (lane >> 5);
    const uint32_t group_lane = lane & 31u;
    const int leader = (int)(lane & ~31u);

    // ---- the group's chunk ----
    const uint64_t f = group / chunks;
    const bool valid = f < (uint64_t)plan->num_bundles;
    uint32_t first_box = 0;     // of the chunk, as a box index of the query
    int32_t num = 0;            // boxes in the chunk, 1 .. 32 (0: no chunk)
    if (valid) {
        const uint32_t first = (uint32_t)(group % chunks) * 32u;    // < per_bundle
        first_box = (uint32_t)f * per_bundle + first;
        num = (int32_t)(per_bundle - first < 32u ? per_bundle - first : 32u);
    }
    const bool has_box = (int32_t)group_lane < num;

    // ---- per bundle, by the group's first lane ----
    BundleHead head { MWHIP_BOXES_OK, 0, 0.f, 0.f, 0.f };
    if (valid && group_lane == 0u) {
        head = readBundle(plan, S, (uint32_t)f);
    }
    // (every lane of the wavefront takes part in the cross-lane reads)
    head.status = __shfl(head.status, leader, 64);
    head.world = __shfl(head.world, leader, 64);
    head.cx = __shfl(head.cx, leader, 64);
    head.cy = __shfl(head.cy, leader, 64);
    head.cz = __shfl(head.cz, leader, 64);

    // ---- per box: lane i has box i of the chunk ----
    int32_t status = head.status;
    math::AABB mine {};
    if (has_box && status == MWHIP_BOXES_OK) {
        status = readBox(plan, first_box + group_lane, head.cx, head.cy, head.cz, &mine);
    }
    const uint32_t open = (uint32_t)wave::groupBallot<32>(has_box && status == MWHIP_BOXES_OK);

    // every lane gets the chunk's boxes (the longer chunk of the two decides
    // how many cross-lane reads the wavefront makes)
    const int32_t num_low = __shfl(num, 0, 64), num_high = __shfl(num, 32, 64);
    const int32_t num_wave = __builtin_amdgcn_readfirstlane(
        num_low > num_high ? num_low : num_high);
    math::AABB boxes[maxBoxes];
    for (int32_t j = 0; j < num_wave; j++) {
        const int src = leader + j;
        boxes[j].pMin.x = __shfl(mine.pMin.x, src, 64);
        boxes[j].pMin.y = __shfl(mine.pMin.y, src, 64);
        boxes[j].pMin.z = __shfl(mine.pMin.z, src, 64);
        boxes[j].pMax.x = __shfl(mine.pMax.x, src, 64);
        boxes[j].pMax.y = __shfl(mine.pMax.y, src, 64);
        boxes[j].pMax.z = __shfl(mine.pMax.z, src, 64);
    }

    // ---- the tree: the two groups part here (worlds differ) ----
    uint32_t count = 0;         // lane j: the running count of box j
    if (open != 0u) {
        Context ctx = TaskGraph::makeContext<Context>(state_mgr, WorldID { head.world });
        const BVH &bvh = ctx.singleton<BVH>();
        if (bvh.numNodes() == 0) {
            // no broadphase pass has built this tree: nothing is met, and the
            // node memory nobody wrote is not walked
        } else if (bvh.needsRebuild()) {
            // (no traversal order: one lane walks the old tree, box after box)
            for (int32_t j = 0; j < num; j++) {
                if ((open >> j & 1u) == 0u) {
                    continue;
                }
                uint32_t n = 0;
                if (group_lane == 0u) {
                    PhysicsSystem::findEntitiesWithinAABB(ctx, boxes[j], [&](Entity e) {
                        if (n < max_hits) {
                            storeHit(plan, first_box + (uint32_t)j, n, e);
                        }
                        n += 1u;
                    });
                }
                n = (uint32_t)__shfl((int32_t)n, leader, 64);
                if ((int32_t)group_lane == j) {
                    count = n;
                }
            }
        } else {
            const int32_t n = bvh.numLeaves();
            const int32_t *order = bvh.traversalOrder();
            for (int32_t base = 0; base < n; base += 32) {
                const int32_t i = base + (int32_t)group_lane;
                Entity e = Entity::none();
                uint32_t hits = 0;
                if (i < n) {
                    const int32_t leaf = order[i];
                    // (the leaf's own box, as findIntersectingLeafBoxes)
                    const math::AABB own = bvh.getLeafAABB(broadphase::LeafID { leaf });
                    uint32_t reached = 0;
                    for (int32_t j = 0; j < num; j++) {
                        if ((open >> j & 1u) != 0u && boxes[j].overlaps(own)) {
                            reached |= 1u << j;
                        }
                    }
                    if (reached != 0u) {
                        e = bvh.leafEntity(leaf);
                        hits = PhysicsSystem::checkEntityAABBsOverlap<maxBoxes>(
                            ctx, boxes, num, reached, e);
                    }
                }
                if (wave::groupBallot<32>(hits != 0u) == 0ull) {
                    continue;
                }
                for (int32_t j = 0; j < num; j++) {
                    const bool hit = (hits >> j & 1u) != 0u;
                    const uint64_t mask = wave::groupBallot<32>(hit);
                    if (mask == 0ull) {
                        continue;
                    }
                    const uint32_t before = (uint32_t)__shfl((int32_t)count, leader + j, 64);
                    const uint32_t rank = before + wave::rankInGroup(mask, group_lane);
                    if (hit && rank < max_hits) {
                        storeHit(plan, first_box + (uint32_t)j, rank, e);
                    }
                    if ((int32_t)group_lane == j) {
                        count += (uint32_t)__builtin_popcountll(mask);
                    }
                }
            }
        }
    }

    // ---- what no entity took, then status and count ----
    for (int32_t j = 0; j < num_wave; j++) {
        const uint32_t got = (uint32_t)__shfl((int32_t)count, leader + j, 64);
        if (j < num) {
            for (uint32_t k = (got < max_hits ? got : max_hits) + group_lane; k < max_hits;
                 k += 32u) {
                storeHit(plan, first_box + (uint32_t)j, k, Entity::none());
            }
        }
    }
    if (has_box) {
        plan->status[first_box + group_lane] = status;
        plan->count[first_box + group_lane] = (int32_t)count;
    }
}

}

__global__ void __launch_bounds__(256)
boxQueryKernel(mwhip_box_args args)
{
    const uint32_t lane = wave::laneID();
    const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    uint32_t total = 0;
#pragma unroll
    for (uint32_t p = 0; p < MWHIP_MAX_STEP_BOXES; p++) {
        if (p < args.num_plans) total += args.items[p];
    }
    for (uint32_t item = blockIdx.x * 4u + wave_in_block; item < total;
         item += gridDim.x * 4u) {
        // the query this item belongs to (constant indices: the arguments stay
        // in scalar registers)
        const mwhip_box_plan *plan = nullptr;
        uint32_t rel = item;
#pragma unroll
        for (uint32_t p = 0; p < MWHIP_MAX_STEP_BOXES; p++) {
            if (plan == nullptr && p < args.num_plans) {
                if (rel < args.items[p]) {
                    plan = args.plans[p];
                } else {
                    rel -= args.items[p];
                }
            }
        }
        if (plan != nullptr) {
            // (the mapping is the same for the whole wavefront)
            if (plan->chunks_per_bundle != 0u) {
                boxq::boxWaveShared(plan, rel, lane);
            } else {
                boxq::boxWavePacked(plan, rel, lane);
            }
        }
    }
}
