// Sort/compaction stress simulator (test workload, not a BASELINE config):
// per-world random create/destroy churn over an archetype whose columns cover
// every gather width of the sort node (1, 2, 4, 8, 12, 16, 20, 240 bytes), plus
// a temporary archetype (makeTemporary / ClearTmpNode / world sort).  Compiled
// unchanged against the reference CPU backend (oracle) and the HIP backend.
#pragma once

#include <madrona/taskgraph_builder.hpp>
#include <madrona/custom_context.hpp>
#include <madrona/rand.hpp>

namespace sortstress {

using madrona::Entity;
using madrona::RandKey;
using madrona::RNG;

namespace consts {
inline constexpr int32_t maxItems = 40;
inline constexpr int32_t maxChurn = 6;
inline constexpr int32_t maxScratch = 12;
// Config::reusePlan: five small archetypes, at most maxReuse rows per world each
inline constexpr int32_t numReuseTables = 5;
inline constexpr int32_t maxReuse = 8;
}

enum class ExportID : uint32_t {
    Churn,
#ifdef MADRONA_GPU_MODE
    Plan,
    Probe,
    ItemVec3,
#endif
    NumExports,
};

struct Tag8 { uint8_t v; };
struct Half { uint16_t v; };
struct Key { uint32_t v; };
struct Pair { uint64_t v; };
struct Vec3 { float v[3]; };
struct Quad { float v[4]; };
struct Blob20 { uint32_t v[5]; };
struct Wide { float v[60]; };

struct Churn {
    uint32_t step;
    uint32_t numItems;
    // written by a system that works in Context::tmpAlloc scratch
    uint32_t scratchSum;
};

#ifdef MADRONA_GPU_MODE
// How a world's Item keys are set by LoadPlan (KeyMode::*, Plan::mode)
enum class KeyMode : uint32_t {
    Random,         // full 32-bit hash values, top bit included
    Equal,          // every key = param
    TwoValues,      // param or ~param
    TopByte,        // only the top byte varies (the rest = param)
    LowByte,        // only the low byte varies (the rest = param)
    Ascending,      // param + 64 * world + slot: ascending in table order
    Descending,     // the complement of Ascending
    AllOnes,        // every key 0xFFFFFFFF
    ZeroOrOnes,     // 0 or 0xFFFFFFFF
    NumModes,
};

// Written by the host (export "plan") before LoadPlan runs: the world's item
// count, how its keys are set, and which of its items are then destroyed
// WITHOUT compaction (bit i: items[i]; their rows stay, WorldID -1).
struct Plan {
    int32_t numItems;
    uint32_t mode;
    uint32_t param;
    uint32_t destroyLo;
    uint32_t destroyHi;
};

// Written by Probe (export "probe"): every item a world holds, read through
// its entity handle (gen, id, Key).
struct ProbeOut {
    int32_t numItems;
    int32_t pad;
    uint32_t items[consts::maxItems][3];
};
#endif

// Task graphs.  Step = the graph every parity test replays.  The other three
// exist on the HIP backend only and split a step so that a test can look at
// the table between nodes: churn WITHOUT compaction (destroyed rows stay),
// SortArchetypeNode<Item, Key> alone (a sort by a non-WorldID key: the
// reference CPU backend's sortArchetype is not an oracle for it),
// and the compaction that has to follow it.
enum class TaskGraphID : uint32_t {
    Step,
#ifdef MADRONA_GPU_MODE
    ChurnOnly,
    SortByKey,
    CompactOnly,
    // Shape-controlled sort tests (tests/test_sort_node_edges_gpu.py):
    // LoadPlan brings every world to its Plan; KeySort / WorldSort are a key
    // sort / compaction each followed by a ResetTmpAlloc that the sort batch
    // may carry; Probe reads every held item's Key through its handle;
    // PlanResize only creates / destroys to Plan::numItems (no compaction:
    // new rows behind the sorted prefix, destroyed ones left in it).
    LoadPlan,
    KeySort,
    WorldSort,
    Probe,
    PlanResize,
    // Config::reusePlan: reusePlanSystem alone, no compaction behind it (rows
    // appended to a table that has not been world-sorted stay that way)
    ReusePlanOnly,
#endif
    NumTaskGraphs,
};

struct Item : public madrona::Archetype<
    Tag8, Half, Key, Pair, Vec3, Quad, Blob20, Wide
> {};

struct Scratch : public madrona::Archetype<
    Key, Vec3
> {};

// Config::reusePlan: rows a world destroys and creates again in one system
struct Reuse0 : public madrona::Archetype<Key, Pair> {};
struct Reuse1 : public madrona::Archetype<Key, Pair> {};
struct Reuse2 : public madrona::Archetype<Key, Pair> {};
struct Reuse3 : public madrona::Archetype<Key, Pair> {};
struct Reuse4 : public madrona::Archetype<Key, Pair> {};

// Config::groupCase: a table that never holds a row
struct Idle : public madrona::Archetype<Key> {};

class Engine;

struct Sim : public madrona::WorldBase {
    struct Config {
        uint32_t seed;
        uint32_t worldBase;
        // 1: some worlds start empty and take their first block of entity ids
        // at run time (ids are then executor-specific; values avoid them)
        uint32_t coldStart;
        // 1: every world starts with one item and only creates until it is
        // full (a population that builds up at run time: table growth)
        uint32_t rampUp;
        // 1: every world logs a message at its second step (more messages in
        // one replay than the executor's message ring holds)
        uint32_t chatty;
        // 1: every world starts with one item; worlds [0, 100) create 30 items
        // at once at their 3rd and 30th step (and destroy them again ten steps
        // later), worlds [200, 264) churn as usual, the rest stand still -- a
        // short tail behind a long sorted prefix in which ONE scatter tile of
        // the compaction chain owns more new rows than it orders in LDS
        uint32_t burst;
        // 1: three more nodes behind the step's last one, all naming the SAME
        // dependency: siblingWriteSystem writes Quad, siblingReadSystem reads
        // Quad (it only comes out right if it runs behind the first, which is
        // the registration order the reference's executors follow),
        // siblingOtherSystem touches Blob20 alone
        uint32_t siblings;
        // 1 (HIP backend only): the Plan / ProbeOut singletons exist and are
        // exported, every world starts with no items (LoadPlan sets the table
        // up).  Off in every parity test: the singletons take entity ids.
        uint32_t plan;
        // 1 (HIP backend only): Item's Vec3 column is exported ("item_vec3"),
        // a pinned column the sort node must keep in place
        uint32_t exportVec3;
        // 1: five more archetypes (Reuse0 .. Reuse4).  In front of the usual
        // step every world destroys a planned subset of their rows and creates
        // a planned number in ONE system (reusePlanSystem), the plan cycling
        // with the global world index and the step: the whole range or a
        // suffix of it with as many, fewer or more creates, a subset that is
        // no suffix, two and five archetypes in one call, a world left with no
        // rows.  On this backend the system is wave-cooperative and asks for
        // OrderedRows::Reuse; the reference build of the same plan uses plain
        // makeEntity / destroyEntity.
        uint32_t reusePlan;
        // 1 .. 5 (HIP backend only): groups named at compile time
        // (madrona::SideBySide) behind the step's last node, one per value --
        // what the runtime must do with them is in sim.cpp, next to the
        // groupCase systems (tests/test_inline_group_fallback_gpu.py)
        uint32_t groupCase;
    };

    struct WorldInit {};

    static void registerTypes(madrona::ECSRegistry &registry,
                              const Config &cfg);
    static void setupTasks(madrona::TaskGraphManager &taskgraph_mgr,
                           const Config &cfg);

    Sim(Engine &ctx, const Config &cfg, const WorldInit &init);

    RNG rng;
    uint32_t mixIds;
    uint32_t rampUp;
    uint32_t chatty;
    uint32_t burst;         // 0: off, 1: a bursting world, 2: churns, 3: stands still
    uint32_t globalWorld;
    int32_t numItems;
    Entity items[consts::maxItems];
    // Config::reusePlan: the world's rows of Reuse0 .. Reuse4, in table order
    int32_t numReuse[consts::numReuseTables];
    Entity reuse[consts::numReuseTables][consts::maxReuse];
};

class Engine : public madrona::CustomContext<Engine, Sim> {
public:
    using CustomContext::CustomContext;
};

}
