#include "sim.hpp"

#ifdef MADRONA_GPU_MODE
#include <madrona/mw_gpu_entry.hpp>
#include <madrona/mw_gpu/host_print.hpp>
#endif

using namespace madrona;

namespace sortstress {

void Sim::registerTypes(ECSRegistry &registry, const Config &cfg)
{
    registry.registerComponent<Tag8>();
    registry.registerComponent<Half>();
    registry.registerComponent<Key>();
    registry.registerComponent<Pair>();
    registry.registerComponent<Vec3>();
    registry.registerComponent<Quad>();
    registry.registerComponent<Blob20>();
    registry.registerComponent<Wide>();
    registry.registerSingleton<Churn>();

    registry.registerArchetype<Item>();
    registry.registerArchetype<Scratch>();

    registry.exportSingleton<Churn>((uint32_t)ExportID::Churn);

    if (cfg.reusePlan != 0) {
        registry.registerArchetype<Reuse0>();
        registry.registerArchetype<Reuse1>();
        registry.registerArchetype<Reuse2>();
        registry.registerArchetype<Reuse3>();
        registry.registerArchetype<Reuse4>();
    }

#ifdef MADRONA_GPU_MODE
    if (cfg.plan != 0) {
        registry.registerSingleton<Plan>();
        registry.registerSingleton<ProbeOut>();
        registry.exportSingleton<Plan>((uint32_t)ExportID::Plan);
        registry.exportSingleton<ProbeOut>((uint32_t)ExportID::Probe);
    }
    if (cfg.exportVec3 != 0) {
        registry.exportColumn<Item, Vec3>((uint32_t)ExportID::ItemVec3);
    }
    if (cfg.groupCase != 0) {
        registry.registerArchetype<Idle>();
    }
#endif
}

static inline void fillItem(Engine &ctx, Entity e, RNG &rng)
{
    uint32_t bits = (uint32_t)rng.sampleI32(0, 0x7FFFFFFF);
    uint32_t id_bits = ctx.data().mixIds != 0 ? (uint32_t)e.id : 0u;

    ctx.get<Tag8>(e).v = (uint8_t)(bits & 0xFF);
    ctx.get<Half>(e).v = (uint16_t)(bits >> 8);
    ctx.get<Key>(e).v = bits;
    ctx.get<Pair>(e).v = ((uint64_t)bits << 32) | (uint64_t)id_bits;

    Vec3 &v3 = ctx.get<Vec3>(e);
    for (int i = 0; i < 3; i++) v3.v[i] = rng.sampleUniform();

    Quad &q = ctx.get<Quad>(e);
    for (int i = 0; i < 4; i++) q.v[i] = (float)i + v3.v[0];

    Blob20 &b = ctx.get<Blob20>(e);
    for (int i = 0; i < 5; i++) b.v[i] = bits * (uint32_t)(i + 1);

    Wide &w = ctx.get<Wide>(e);
    for (int i = 0; i < 60; i++) w.v[i] = (float)(bits & 0xFFFF) + (float)i;
}

inline void churnSystem(Engine &ctx, Churn &churn)
{
    Sim &sim = ctx.data();
    RNG &rng = sim.rng;

    if (sim.burst == 1u || sim.burst == 3u) {
        // burst mode: no churn; the bursting worlds fill up at steps 3 and 30
        // and empty again at steps 13 and 40
        if (sim.burst == 1u && (churn.step == 2u || churn.step == 29u)) {
            while (sim.numItems < 31) {
                Entity e = ctx.makeEntity<Item>();
                fillItem(ctx, e, rng);
                sim.items[sim.numItems++] = e;
            }
        }
        if (sim.burst == 1u && (churn.step == 12u || churn.step == 39u)) {
            while (sim.numItems > 1) {
                ctx.destroyEntity(sim.items[--sim.numItems]);
            }
        }
        churn.step += 1;
        churn.numItems = (uint32_t)sim.numItems;
        return;
    }

    int32_t num_destroy = rng.sampleI32(0, consts::maxChurn + 1);
    if (sim.rampUp != 0 && sim.numItems < consts::maxItems) {
        num_destroy = 0;
    }
    for (int32_t i = 0; i < num_destroy && sim.numItems > 0; i++) {
        int32_t victim = rng.sampleI32(0, sim.numItems);
        ctx.destroyEntity(sim.items[victim]);
        sim.items[victim] = sim.items[sim.numItems - 1];
        sim.numItems -= 1;
    }

    int32_t num_create = rng.sampleI32(0, consts::maxChurn + 1);
    for (int32_t i = 0; i < num_create && sim.numItems < consts::maxItems; i++) {
        Entity e = ctx.makeEntity<Item>();
        fillItem(ctx, e, rng);
        sim.items[sim.numItems++] = e;
    }

    int32_t num_scratch = rng.sampleI32(0, consts::maxScratch + 1);
    for (int32_t i = 0; i < num_scratch; i++) {
        Loc loc = ctx.makeTemporary<Scratch>();
        ctx.get<Key>(loc).v = churn.step * 1000u + (uint32_t)i;
        Vec3 &v = ctx.get<Vec3>(loc);
        v.v[0] = rng.sampleUniform();
        v.v[1] = (float)i;
        v.v[2] = (float)churn.step;
    }

    churn.step += 1;
    churn.numItems = (uint32_t)sim.numItems;

#ifdef MADRONA_GPU_MODE
    // device-side printf through the executor's message ring (every argument
    // type the channel carries); world 3 speaks once, at its third step
    if (ctx.worldID().idx == 3 && churn.step == 3u) {
        mwGPU::HostPrint::log(
            "sort_stress: world {} step {} items {} mean {} key {} ptr {}",
            ctx.worldID().idx, churn.step, (int64_t)sim.numItems,
            (float)sim.numItems * 0.5f, (uint64_t)0x123456789ABCull,
            (void *)&sim);
    }
    if (sim.chatty != 0 && churn.step == 2u) {
        mwGPU::HostPrint::log("sort_stress: chatty world {}", ctx.worldID().idx);
    }
#endif
}

inline void touchSystem(Engine &ctx, Entity e, Key &key, Vec3 &v3, Wide &wide)
{
    uint32_t id_bits = ctx.data().mixIds != 0 ? (uint32_t)e.id : 0u;
    key.v = key.v * 1664525u + 1013904223u + id_bits;
    v3.v[1] = v3.v[1] * 0.5f + 0.25f;
    wide.v[(key.v >> 8) % 60] += 1.f;
}

inline void scratchSystem(Engine &ctx, Key &key, Vec3 &v3)
{
    v3.v[2] = v3.v[2] + (float)ctx.worldID().idx + (float)(key.v & 7u);
}

// The same per-row update twice: as an items_per_invocation = 4
// CustomParallelForNode (Fn(WorldID *, Cs *..., count), reference device
// taskgraph.inl:229-266 -- that node type only exists in the reference's
// device headers) and, for the CPU oracle, as an ordinary ParallelForNode.
static inline void scaleOne(Half &h, Pair &p)
{
    h.v = (uint16_t)(h.v * 3u + 1u);
    p.v += (uint64_t)h.v << 8;
}

#ifdef MADRONA_GPU_MODE
inline void scaleBatch(WorldID *worlds, Half *halves, Pair *pairs,
                       int32_t count)
{
    for (int32_t i = 0; i < count; i++) {
        if (worlds[i].idx != -1) {
            scaleOne(halves[i], pairs[i]);
        }
    }
}
#else
inline void scaleSystem(Engine &, Half &h, Pair &p)
{
    scaleOne(h, p);
}
#endif

// Works in per-step scratch memory (Context::tmpAlloc; freed by
// ResetTmpAllocNode): fills a buffer, reads it back in another order.
inline void scratchSumSystem(Engine &ctx, Churn &churn)
{
    constexpr int32_t n = 24;
    uint32_t *buf = (uint32_t *)ctx.tmpAlloc(sizeof(uint32_t) * n);
    for (int32_t i = 0; i < n; i++) {
        buf[i] = churn.step * 2654435761u + (uint32_t)i * 40503u +
            churn.numItems;
    }
    uint32_t sum = 0;
    for (int32_t i = n - 1; i >= 0; i--) {
        sum = sum * 31u + buf[i];
    }
    churn.scratchSum = sum;
}

// Three nodes that name the same dependency (Config::siblings).  The second
// reads what the first writes: right only behind it.  The reference runs nodes
// in registration order whatever they declared; this backend runs nodes with
// equal dependencies in one launch UNLESS their signatures clash (a non-const
// reference to a component the other names, on a shared table) -- the first two
// must stay apart, the last two may share a launch.
inline void siblingWriteSystem(Engine &, Quad &q)
{
    q.v[0] = q.v[0] * 0.5f + 1.f;
}

inline void siblingReadSystem(Engine &, const Quad &q, Vec3 &v)
{
    v.v[2] = q.v[0] + q.v[1];
}

inline void siblingOtherSystem(Engine &, Blob20 &b)
{
    b.v[4] += 3u;
}

#ifdef MADRONA_GPU_MODE
// ---- groups named at compile time (Config::groupCase) ------------------------
// SideBySide groups behind the step's last node; what has to come of each:
//   1  idle | blob         one member's table (Idle) has no rows: one launch
//   2  churnTag | blob     with one world churnTag has ONE row: one launch
//   3  blob | wide32 | quad64   1, 32 and 64 lanes per row: one launch
//   4  siblingWrite | siblingRead   clash on Quad: two launches, in this order
//   5  appender | blob     appender can append rows (it never does): its own
//                          launch, and blob alone keeps its own as well
inline void groupIdleSystem(Engine &, Key &key)
{
    key.v += 1u;
}

inline void groupBlobSystem(Engine &, Blob20 &b)
{
    b.v[3] = b.v[3] * 3u + 1u;
}

inline void groupChurnTagSystem(Engine &, Churn &churn)
{
    churn.scratchSum ^= 0x5A5A0000u + churn.step;
}

// lane l of 32 owns Wide::v[l]
inline void groupWide32System(Engine &, Wide &w)
{
    const uint32_t lane = threadIdx.x % 32u;
    w.v[lane] = w.v[lane] * 0.5f + (float)lane;
}

// lanes 0 .. 3 of 64 own Quad::v[l]
inline void groupQuad64System(Engine &, Quad &q)
{
    const uint32_t lane = threadIdx.x % 64u;
    if (lane < 4u) {
        q.v[lane] = q.v[lane] * 0.25f + (float)lane;
    }
}

// (carries the row appender's marker; no world reaches step 0xFFFFFFFF)
inline void groupAppenderSystem(Engine &ctx, Churn &churn)
{
    if (churn.step == 0xFFFFFFFFu) {
        Loc loc = ctx.makeTemporary<Scratch>();
        ctx.get<Key>(loc).v = 0u;
    }
    churn.scratchSum += 7u;
}

// ---- shape-controlled sort tests (Config::plan) ----------------------------
static inline uint32_t mixBits(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

static inline uint32_t planKey(const Plan &plan, uint32_t world, uint32_t slot)
{
    const uint32_t ordinal = world * 64u + slot;
    const uint32_t h = mixBits(plan.param ^ mixBits(ordinal + 0x9E3779B9u));
    switch ((KeyMode)plan.mode) {
    case KeyMode::Random: return h;
    case KeyMode::Equal: return plan.param;
    case KeyMode::TwoValues: return (h & 1u) != 0u ? ~plan.param : plan.param;
    case KeyMode::TopByte: return (h & 0xFF000000u) | (plan.param & 0x00FFFFFFu);
    case KeyMode::LowByte: return (plan.param & 0xFFFFFF00u) | (h & 0xFFu);
    case KeyMode::Ascending: return plan.param + ordinal;
    case KeyMode::Descending: return ~(plan.param + ordinal);
    case KeyMode::AllOnes: return 0xFFFFFFFFu;
    case KeyMode::ZeroOrOnes: return (h & 1u) != 0u ? 0xFFFFFFFFu : 0u;
    default: return h;
    }
}

// Brings the world to plan.numItems items (destroys from the back, creates new
// ones behind); the compaction that follows makes the table world-major.
inline void planResizeSystem(Engine &ctx, Plan &plan)
{
    Sim &sim = ctx.data();
    int32_t target = plan.numItems < 0 ? 0 :
        (plan.numItems > consts::maxItems ? consts::maxItems : plan.numItems);
    while (sim.numItems > target) {
        ctx.destroyEntity(sim.items[--sim.numItems]);
    }
    while (sim.numItems < target) {
        Entity e = ctx.makeEntity<Item>();
        fillItem(ctx, e, sim.rng);
        sim.items[sim.numItems++] = e;
    }
}

// Keys by plan.mode, then the items the plan names are destroyed: their rows
// stay in the table (WorldID -1) until the next compaction.
inline void planKeysSystem(Engine &ctx, Plan &plan)
{
    Sim &sim = ctx.data();
    for (int32_t i = 0; i < sim.numItems; i++) {
        ctx.get<Key>(sim.items[i]).v = planKey(plan, sim.globalWorld, (uint32_t)i);
    }
    int32_t kept = 0;
    for (int32_t i = 0; i < sim.numItems; i++) {
        const uint32_t bit = i < 32 ? (plan.destroyLo >> i) & 1u :
            (plan.destroyHi >> (i - 32)) & 1u;
        if (bit != 0u) {
            ctx.destroyEntity(sim.items[i]);
        } else {
            sim.items[kept++] = sim.items[i];
        }
    }
    sim.numItems = kept;
}

// Every held item's Key read through its entity handle (the Loc a sort left).
inline void probeSystem(Engine &ctx, ProbeOut &out)
{
    Sim &sim = ctx.data();
    out.numItems = sim.numItems;
    out.pad = 0;
    for (int32_t i = 0; i < consts::maxItems; i++) {
        if (i < sim.numItems) {
            Entity e = sim.items[i];
            out.items[i][0] = e.gen;
            out.items[i][1] = (uint32_t)e.id;
            out.items[i][2] = ctx.get<Key>(e).v;
        } else {
            out.items[i][0] = 0xFFFFFFFFu;
            out.items[i][1] = 0xFFFFFFFFu;
            out.items[i][2] = 0u;
        }
    }
}
#endif

// ---- Config::reusePlan ------------------------------------------------------
struct ReusePlan {
    uint32_t destroy[consts::numReuseTables];   // bit i: the world's i-th row
    int32_t create[consts::numReuseTables];
};

static inline uint32_t reuseMix(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// the last k of n rows
static inline uint32_t reuseSuffix(int32_t n, int32_t k)
{
    return ((1u << n) - 1u) & ~((1u << (n - k)) - 1u);
}

static inline int32_t reuseBits(uint32_t x)
{
    int32_t n = 0;
    for (; x != 0u; x &= x - 1u) n++;
    return n;
}

// What the world does to its Reuse tables at this step.  Rows are named by
// their position in the world's list, which is their order in the table:
// survivors keep their order, new rows follow in creation order.
static inline ReusePlan reusePlanFor(const Sim &sim, uint32_t step)
{
    ReusePlan p {};
    const int32_t n0 = sim.numReuse[0];
    const int32_t half = (n0 + 1) / 2;
    switch ((sim.globalWorld + step) % 8u) {
    case 0:     // the whole range, as many again
        p.destroy[0] = reuseSuffix(n0, n0);
        p.create[0] = n0;
        break;
    case 1:     // a proper suffix, as many again
        p.destroy[0] = reuseSuffix(n0, half);
        p.create[0] = half;
        break;
    case 2:     // a suffix, fewer creates
        p.destroy[0] = reuseSuffix(n0, half);
        p.create[0] = half > 0 ? half - 1 : 0;
        break;
    case 3:     // a suffix, more creates: reuse and append in one call
        p.destroy[0] = reuseSuffix(n0, half);
        p.create[0] = half + 2;
        break;
    case 4:     // no suffix: the first row of several
        p.destroy[0] = n0 >= 2 ? 1u : 0u;
        p.create[0] = 1;
        break;
    case 5:     // two archetypes in one call
        p.destroy[0] = reuseSuffix(n0, half);
        p.create[0] = half;
        p.destroy[1] = reuseSuffix(sim.numReuse[1], sim.numReuse[1]);
        p.create[1] = sim.numReuse[1];
        break;
    case 6:     // five archetypes in one call: the last row of each
        for (int32_t a = 0; a < consts::numReuseTables; a++) {
            p.destroy[a] = reuseSuffix(sim.numReuse[a], sim.numReuse[a] > 0 ? 1 : 0);
            p.create[a] = 1;
        }
        break;
    default:    // leaves the world without rows in the first table
        p.destroy[0] = reuseSuffix(n0, n0);
        p.create[0] = 0;
        break;
    }
    for (int32_t a = 0; a < consts::numReuseTables; a++) {
        const int32_t room =
            consts::maxReuse - (sim.numReuse[a] - reuseBits(p.destroy[a]));
        if (p.create[a] > room) {
            p.create[a] = room;
        }
    }
    return p;
}

static inline uint32_t reuseKey(const Sim &sim, uint32_t step, int32_t a, int32_t j)
{
    return reuseMix(sim.globalWorld * 977u + step * 31u + (uint32_t)(a * 8 + j));
}

#ifdef MADRONA_GPU_MODE
static inline uint32_t reuseArchetype(int32_t a)
{
    switch (a) {
    case 0: return TypeTracker::typeID<Reuse0>();
    case 1: return TypeTracker::typeID<Reuse1>();
    case 2: return TypeTracker::typeID<Reuse2>();
    case 3: return TypeTracker::typeID<Reuse3>();
    default: return TypeTracker::typeID<Reuse4>();
    }
}

// 64 lanes per world (CustomParallelForNode<..., 64, 1>): lane 8 a + i stands
// for row i of table a.  The same ids, rows and values as the loops below.
inline void reusePlanSystem(Engine &ctx, Churn &churn)
{
    Sim &sim = ctx.data();
    const ReusePlan plan = reusePlanFor(sim, churn.step);

    const int32_t lane = (int32_t)(threadIdx.x % 64);
    const bool on_table = lane < consts::numReuseTables * consts::maxReuse;
    const int32_t a = on_table ? lane / consts::maxReuse : 0;
    const int32_t i = lane % consts::maxReuse;
    const int32_t n = sim.numReuse[a];
    const bool held = on_table && i < n;
    const Entity mine = held ? sim.reuse[a][i] : Entity::none();
    const bool gone = held && ((plan.destroy[a] >> i) & 1u) != 0u;
    const int32_t kept = n - reuseBits(plan.destroy[a]);
    const int32_t kept_before =
        reuseBits(~plan.destroy[a] & ((1u << i) - 1u) & ((1u << n) - 1u));

    ctx.destroyEntityOrdered(mine, gone, OrderedRows::Reuse);

    const bool make = on_table && i < plan.create[a];
    const Entity e = ctx.makeEntityOrdered(reuseArchetype(a), make, OrderedRows::Reuse);
    if (make) {
        const uint32_t key = reuseKey(sim, churn.step, a, i);
        ctx.get<Key>(e).v = key;
        ctx.get<Pair>(e).v = ((uint64_t)key << 32) | (uint64_t)(uint32_t)i;
    }

    // (every lane read its own slot above; the slots written are distinct)
    if (held && !gone) {
        sim.reuse[a][kept_before] = mine;
    }
    if (make) {
        sim.reuse[a][kept + i] = e;
    }
    if (on_table && i == 0) {
        sim.numReuse[a] = kept + plan.create[a];
    }
}
#else
template <typename ArchetypeT>
static inline void reusePlanTable(Engine &ctx, Sim &sim, const ReusePlan &plan,
                                  uint32_t step, int32_t a, bool destroy)
{
    if (destroy) {
        int32_t kept = 0;
        for (int32_t i = 0; i < sim.numReuse[a]; i++) {
            if (((plan.destroy[a] >> i) & 1u) != 0u) {
                ctx.destroyEntity(sim.reuse[a][i]);
            } else {
                sim.reuse[a][kept++] = sim.reuse[a][i];
            }
        }
        sim.numReuse[a] = kept;
        return;
    }
    for (int32_t j = 0; j < plan.create[a]; j++) {
        Entity e = ctx.makeEntity<ArchetypeT>();
        const uint32_t key = reuseKey(sim, step, a, j);
        ctx.get<Key>(e).v = key;
        ctx.get<Pair>(e).v = ((uint64_t)key << 32) | (uint64_t)(uint32_t)j;
        sim.reuse[a][sim.numReuse[a]++] = e;
    }
}

inline void reusePlanSystem(Engine &ctx, Churn &churn)
{
    Sim &sim = ctx.data();
    const ReusePlan plan = reusePlanFor(sim, churn.step);
    for (int32_t pass = 0; pass < 2; pass++) {
        const bool destroy = pass == 0;
        reusePlanTable<Reuse0>(ctx, sim, plan, churn.step, 0, destroy);
        reusePlanTable<Reuse1>(ctx, sim, plan, churn.step, 1, destroy);
        reusePlanTable<Reuse2>(ctx, sim, plan, churn.step, 2, destroy);
        reusePlanTable<Reuse3>(ctx, sim, plan, churn.step, 3, destroy);
        reusePlanTable<Reuse4>(ctx, sim, plan, churn.step, 4, destroy);
    }
}
#endif

template <typename ArchetypeT>
static inline void reuseInitTable(Engine &ctx, Sim &sim, int32_t a)
{
    const int32_t initial = (int32_t)((sim.globalWorld * 3u + (uint32_t)a * 2u) % 6u);
    sim.numReuse[a] = 0;
    for (int32_t j = 0; j < initial; j++) {
        Entity e = ctx.makeEntity<ArchetypeT>();
        const uint32_t key = reuseKey(sim, 0xFFFFu, a, j);
        ctx.get<Key>(e).v = key;
        ctx.get<Pair>(e).v = ((uint64_t)key << 32) | (uint64_t)(uint32_t)j;
        sim.reuse[a][sim.numReuse[a]++] = e;
    }
}

void Sim::setupTasks(TaskGraphManager &taskgraph_mgr, const Config &cfg)
{
    TaskGraphBuilder &builder = taskgraph_mgr.init(TaskGraphID::Step);

    auto clear_tmp = builder.addToGraph<ClearTmpNode<Scratch>>({});
    if (cfg.reusePlan != 0) {
#ifdef MADRONA_GPU_MODE
        auto plan_sys = builder.addToGraph<CustomParallelForNode<Engine,
            reusePlanSystem, 64, 1, Churn>>({clear_tmp});
#else
        auto plan_sys = builder.addToGraph<ParallelForNode<Engine,
            reusePlanSystem, Churn>>({clear_tmp});
#endif
        auto c0 = builder.addToGraph<CompactArchetypeNode<Reuse0>>({plan_sys});
        auto c1 = builder.addToGraph<CompactArchetypeNode<Reuse1>>({c0});
        auto c2 = builder.addToGraph<CompactArchetypeNode<Reuse2>>({c1});
        auto c3 = builder.addToGraph<CompactArchetypeNode<Reuse3>>({c2});
        clear_tmp = builder.addToGraph<CompactArchetypeNode<Reuse4>>({c3});
    }

    auto churn_sys = builder.addToGraph<ParallelForNode<Engine,
        churnSystem, Churn>>({clear_tmp});

    auto compact = builder.addToGraph<CompactArchetypeNode<Item>>({churn_sys});

#ifdef MADRONA_GPU_MODE
    // as the reference's XPBD graph does for Contact temporaries
    // (src/physics/xpbd.cpp:1107-1113): group temporaries by world
    auto sort_tmp = builder.addToGraph<
        SortArchetypeNode<Scratch, WorldID>>({compact});
    auto post_sort = builder.addToGraph<ResetTmpAllocNode>({sort_tmp});
#else
    auto post_sort = compact;
#endif

    auto touch_sys = builder.addToGraph<ParallelForNode<Engine,
        touchSystem, Entity, Key, Vec3, Wide>>({post_sort});

    auto scratch_sys = builder.addToGraph<ParallelForNode<Engine,
        scratchSystem, Key, Vec3>>({touch_sys});

#ifdef MADRONA_GPU_MODE
    auto scale_sys = builder.addToGraph<CustomParallelForNode<Engine,
        scaleBatch, 1, 4, Half, Pair>>({scratch_sys});
#else
    auto scale_sys = builder.addToGraph<ParallelForNode<Engine,
        scaleSystem, Half, Pair>>({scratch_sys});
#endif

    auto sum_sys = builder.addToGraph<ParallelForNode<Engine,
        scratchSumSystem, Churn>>({scale_sys});
    auto reset_tmp = builder.addToGraph<ResetTmpAllocNode>({sum_sys});
    if (cfg.siblings != 0) {
        builder.addToGraph<ParallelForNode<Engine,
            siblingWriteSystem, Quad>>({reset_tmp});
        builder.addToGraph<ParallelForNode<Engine,
            siblingReadSystem, Quad, Vec3>>({reset_tmp});
        builder.addToGraph<ParallelForNode<Engine,
            siblingOtherSystem, Blob20>>({reset_tmp});
    }

#ifdef MADRONA_GPU_MODE
    using BlobNode = ParallelForNode<Engine, groupBlobSystem, Blob20>;
    switch (cfg.groupCase) {
    case 1:
        SideBySide<ParallelForNode<Engine, groupIdleSystem, Key>,
                   BlobNode>::addToGraph(builder, {reset_tmp});
        break;
    case 2:
        SideBySide<ParallelForNode<Engine, groupChurnTagSystem, Churn>,
                   BlobNode>::addToGraph(builder, {reset_tmp});
        break;
    case 3:
        SideBySide<BlobNode,
                   CustomParallelForNode<Engine, groupWide32System, 32, 1, Wide>,
                   CustomParallelForNode<Engine, groupQuad64System, 64, 1, Quad>
                  >::addToGraph(builder, {reset_tmp});
        break;
    case 4:
        SideBySide<ParallelForNode<Engine, siblingWriteSystem, Quad>,
                   ParallelForNode<Engine, siblingReadSystem, Quad, Vec3>
                  >::addToGraph(builder, {reset_tmp});
        break;
    case 5:
        SideBySide<ParallelForNode<Engine, groupAppenderSystem, Churn>,
                   BlobNode>::addToGraph(builder, {reset_tmp});
        break;
    default:
        break;
    }
#endif

#ifdef MADRONA_GPU_MODE
    {
        TaskGraphBuilder &b = taskgraph_mgr.init(TaskGraphID::ChurnOnly);
        auto clear = b.addToGraph<ClearTmpNode<Scratch>>({});
        b.addToGraph<ParallelForNode<Engine, churnSystem, Churn>>({clear});
    }
    {
        TaskGraphBuilder &b = taskgraph_mgr.init(TaskGraphID::SortByKey);
        b.addToGraph<SortArchetypeNode<Item, Key>>({});
    }
    {
        TaskGraphBuilder &b = taskgraph_mgr.init(TaskGraphID::CompactOnly);
        auto c = b.addToGraph<CompactArchetypeNode<Item>>({});
        b.addToGraph<SortArchetypeNode<Scratch, WorldID>>({c});
    }
    {
        TaskGraphBuilder &b = taskgraph_mgr.init(TaskGraphID::LoadPlan);
        if (cfg.plan != 0) {
            auto resize = b.addToGraph<ParallelForNode<Engine,
                planResizeSystem, Plan>>({});
            auto c = b.addToGraph<CompactArchetypeNode<Item>>({resize});
            b.addToGraph<ParallelForNode<Engine, planKeysSystem, Plan>>({c});
        } else {
            b.addToGraph<ResetTmpAllocNode>({});
        }
    }
    {
        TaskGraphBuilder &b = taskgraph_mgr.init(TaskGraphID::KeySort);
        auto sort = b.addToGraph<SortArchetypeNode<Item, Key>>({});
        b.addToGraph<ResetTmpAllocNode>({sort});
    }
    {
        TaskGraphBuilder &b = taskgraph_mgr.init(TaskGraphID::WorldSort);
        auto c = b.addToGraph<CompactArchetypeNode<Item>>({});
        b.addToGraph<ResetTmpAllocNode>({c});
    }
    {
        TaskGraphBuilder &b = taskgraph_mgr.init(TaskGraphID::Probe);
        if (cfg.plan != 0) {
            b.addToGraph<ParallelForNode<Engine, probeSystem, ProbeOut>>({});
        } else {
            b.addToGraph<ResetTmpAllocNode>({});
        }
    }
    {
        TaskGraphBuilder &b = taskgraph_mgr.init(TaskGraphID::ReusePlanOnly);
        if (cfg.reusePlan != 0) {
            b.addToGraph<CustomParallelForNode<Engine,
                reusePlanSystem, 64, 1, Churn>>({});
        } else {
            b.addToGraph<ResetTmpAllocNode>({});
        }
    }
    {
        TaskGraphBuilder &b = taskgraph_mgr.init(TaskGraphID::PlanResize);
        if (cfg.plan != 0) {
            b.addToGraph<ParallelForNode<Engine, planResizeSystem, Plan>>({});
        } else {
            b.addToGraph<ResetTmpAllocNode>({});
        }
    }
#endif
}

Sim::Sim(Engine &ctx, const Config &cfg, const WorldInit &)
    : WorldBase(ctx)
{
    uint32_t global_world = cfg.worldBase + (uint32_t)ctx.worldID().idx;
    rng = RNG(rand::split_i(rand::initKey(cfg.seed), global_world));
    mixIds = cfg.coldStart == 0 ? 1u : 0u;
    rampUp = cfg.rampUp;
    chatty = cfg.chatty;
    numItems = 0;

    Churn &churn = ctx.singleton<Churn>();
    churn.step = 0;
    churn.numItems = 0;
    churn.scratchSum = 0;

    // ragged start; with coldStart some worlds begin empty
    int32_t initial = cfg.coldStart != 0 ?
        (int32_t)((global_world * 7u) % (uint32_t)consts::maxItems) :
        1 + (int32_t)((global_world * 7u) % (uint32_t)(consts::maxItems - 1));
    if (cfg.rampUp != 0 || cfg.burst != 0) {
        initial = 1;
    }
    globalWorld = global_world;
#ifdef MADRONA_GPU_MODE
    if (cfg.plan != 0) {
        initial = 0;
        ctx.singleton<Plan>() = Plan {};
        ctx.singleton<ProbeOut>() = ProbeOut {};
    }
#endif
    burst = 0;
    if (cfg.burst != 0) {
        burst = global_world < 100u ? 1u :
            (global_world >= 200u && global_world < 264u) ? 2u : 3u;
    }
    for (int32_t i = 0; i < initial; i++) {
        Entity e = ctx.makeEntity<Item>();
        fillItem(ctx, e, rng);
        items[numItems++] = e;
    }
    for (int32_t a = 0; a < consts::numReuseTables; a++) {
        numReuse[a] = 0;
    }
    if (cfg.reusePlan != 0) {
        reuseInitTable<Reuse0>(ctx, *this, 0);
        reuseInitTable<Reuse1>(ctx, *this, 1);
        reuseInitTable<Reuse2>(ctx, *this, 2);
        reuseInitTable<Reuse3>(ctx, *this, 3);
        reuseInitTable<Reuse4>(ctx, *this, 4);
    }
}

#ifdef MADRONA_GPU_MODE
MADRONA_BUILD_MWGPU_ENTRY(Engine, Sim, Sim::Config, Sim::WorldInit);
#endif

}
