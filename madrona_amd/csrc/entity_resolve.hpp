// From an entity handle in device memory to the row it names, as
// Context::get<T>(e) goes but trusting no bit of the handle: shared by the entity
// gathers (entityGatherKernel, entity_gather.hip), which read the cells of that
// row, and the entity scatters (scatterClaimKernel / scatterWriteKernel,
// entity_scatter.hip), which write them.  The rule is gather_ref.py's (DESIGN.md
// §31).  Device code of libmadrona_hip.so; included behind exec_internal.hpp
// (EcsState, TableHdr, EntitySlot); not installed.
#pragma once
#include "copy_chunk.hpp"

#include <cstddef>

namespace madrona {
namespace mwhip {

// Where the handles are (mwhip_gather_source): a run of records with a run of
// 8-byte Entity cells in each.  Part of a device-resident plan.
struct HandleSource {
    const char *src;        // the caller's: records of recordBytes, 4-byte aligned
    uint32_t recordBytes;
    uint32_t firstByte;
    uint32_t perRecord;
    uint32_t pad_;
};

// Where a handle's entity is, if it names one.
struct Resolved {
    int32_t archetype;      // -1: names nothing
    int32_t world;
    int32_t row;
    int32_t id;             // the handle's, whatever it names
};

// Handle i of `source` (valid: i is one of its handles).  The handle is loaded
// as two dwords (the source is 4-byte aligned, no more) and nothing is
// dereferenced behind a check that failed: 0 <= id < entityCapacity, slot.gen ==
// gen, archetype < numArchetypeSlots and registered, 0 <= row < numRows, the
// row's own Entity cell == the handle and its WorldID cell != -1 (a statement
// about the TABLES: the slot only says where to look).
__device__ inline Resolved resolveHandle(const EcsState *S, const HandleSource &source,
                                         uint32_t i, bool valid)
{
    Resolved out = { -1, -1, 0, -1 };
    if (!valid) return out;

    const uint32_t per = source.perRecord;
    const uint32_t rec = i / per;
    const uint32_t k = i - rec * per;
    const GlobalU32 *h = (const GlobalU32 *)(uint64_t)(
        source.src + (uint64_t)rec * source.recordBytes + source.firstByte + (uint64_t)k * 8ull);
    const uint32_t gen = h[0];
    const int32_t id = (int32_t)h[1];
    out.id = id;

    // (the device copy: the store may have grown since the plan was made)
    if (id < 0 || id >= S->entityCapacity) return out;
    const GlobalU32 *slot = (const GlobalU32 *)(uint64_t)(S->entities + id);
    static_assert(sizeof(EntitySlot) == 12 && offsetof(EntitySlot, gen) == 8);
    const uint32_t archetype = slot[0];
    const int32_t row = (int32_t)slot[1];
    // a stale handle, or a free slot (whose first two words are list links)
    if (slot[2] != gen) return out;

    // a free slot whose generation the handle happens to carry: its "archetype"
    // and "row" are free-list links
    if (archetype >= S->numArchetypeSlots) return out;
    const TableHdr *hdr = S->tables + archetype;
    if (hdr->registered == 0u) return out;
    if (row < 0 || row >= hdr->numRows) return out;

    // the row itself has the last word: it holds this entity, and it is live
    const GlobalU32 *cell = (const GlobalU32 *)(uint64_t)hdr->columns[0] + 2ull * (uint32_t)row;
    const int32_t world = ((const int32_t *)hdr->columns[1])[row];
    if (cell[0] != gen || (int32_t)cell[1] != id || world == -1) return out;

    out.archetype = (int32_t)archetype;
    out.world = world;
    out.row = row;
    return out;
}

}
}
