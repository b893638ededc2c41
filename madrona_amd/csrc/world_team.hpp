// What a TEAM of lanes of one wavefront does for one world of a table: shared
// by the world views (worldViewKernel, world_view.hip), which copy a world's
// rows out of the table, and the world writes (worldWriteKernel,
// world_write.hip), which copy them in; the entity gathers (entityGatherKernel,
// entity_gather.hip) and the entity scatters (scatterWriteKernel,
// entity_scatter.hip) copy single cells with the same teams.  A team is T lanes (a power of two,
// 1 .. 64) of a wavefront; t is a lane's number in its team.  Device code of
// libmadrona_hip.so; included behind exec_internal.hpp (TableHdr); not installed.
#pragma once
#include "copy_chunk.hpp"

namespace madrona {
namespace mwhip {

// n bytes by the T lanes of a team: 16 bytes per lane where source and
// destination agree modulo 16, dwords where they agree modulo 4, bytes
// otherwise, with a peeled head up to the first aligned address
__device__ inline void teamCopy(char *dst, const char *src, uint64_t n, uint32_t t, uint32_t T)
{
    const uint64_t d = (uint64_t)dst, s = (uint64_t)src;
    GlobalU8 *d8 = (GlobalU8 *)d;
    const GlobalU8 *s8 = (const GlobalU8 *)s;
    uint64_t done = 0;
    if (((d ^ s) & 15ull) == 0ull) {
        uint64_t head = (16ull - (d & 15ull)) & 15ull;
        head = head < n ? head : n;
        for (uint64_t i = t; i < head; i += T) d8[i] = s8[i];
        const uint64_t num_vec = (n - head) >> 4;
        GlobalU4 *d4 = (GlobalU4 *)(d + head);
        const GlobalU4 *s4 = (const GlobalU4 *)(s + head);
        for (uint64_t i = t; i < num_vec; i += T) d4[i] = s4[i];
        done = head + (num_vec << 4);
    } else if (((d ^ s) & 3ull) == 0ull) {
        uint64_t head = (4ull - (d & 3ull)) & 3ull;
        head = head < n ? head : n;
        for (uint64_t i = t; i < head; i += T) d8[i] = s8[i];
        const uint64_t num_words = (n - head) >> 2;
        GlobalU32 *d1 = (GlobalU32 *)(d + head);
        const GlobalU32 *s1 = (const GlobalU32 *)(s + head);
        for (uint64_t i = t; i < num_words; i += T) d1[i] = s1[i];
        done = head + (num_words << 2);
    }
    for (uint64_t i = done + t; i < n; i += T) d8[i] = s8[i];
}

// n zero bytes by the T lanes of a team
__device__ inline void teamZero(char *dst, uint64_t n, uint32_t t, uint32_t T)
{
    const uint64_t d = (uint64_t)dst;
    GlobalU8 *d8 = (GlobalU8 *)d;
    uint64_t head = (16ull - (d & 15ull)) & 15ull;
    head = head < n ? head : n;
    for (uint64_t i = t; i < head; i += T) d8[i] = (uint8_t)0;
    const uint64_t num_vec = (n - head) >> 4;
    GlobalU4 *d4 = (GlobalU4 *)(d + head);
    const CopyU4 zero = { 0u, 0u, 0u, 0u };
    for (uint64_t i = t; i < num_vec; i += T) d4[i] = zero;
    for (uint64_t i = head + (num_vec << 4) + t; i < n; i += T) d8[i] = (uint8_t)0;
}

// one cell by one lane
__device__ inline void cellCopy(char *dst, const char *src, uint32_t bytes)
{
    const uint64_t d = (uint64_t)dst, s = (uint64_t)src;
    if (((d | s) & 15ull) == 0ull && bytes % 16u == 0u) {
        GlobalU4 *d4 = (GlobalU4 *)d;
        const GlobalU4 *s4 = (const GlobalU4 *)s;
        for (uint32_t i = 0; i < bytes / 16u; i++) d4[i] = s4[i];
    } else if (((d | s) & 3ull) == 0ull && bytes % 4u == 0u) {
        GlobalU32 *d1 = (GlobalU32 *)d;
        const GlobalU32 *s1 = (const GlobalU32 *)s;
        for (uint32_t i = 0; i < bytes / 4u; i++) d1[i] = s1[i];
    } else {
        GlobalU8 *d8 = (GlobalU8 *)d;
        const GlobalU8 *s8 = (const GlobalU8 *)s;
        for (uint32_t i = 0; i < bytes; i++) d8[i] = s8[i];
    }
}

// Where a team looks for world w's rows, read from the table's header when the
// kernel runs: rows [lo, hi) of the sorted prefix [0, prefix) -- a HINT, every
// row is still tested against its own WorldID cell -- and then all of
// [prefix, n).  0 <= lo <= hi <= prefix <= n, whatever the header says.
struct TeamRange {
    int32_t lo;
    int32_t hi;
    int32_t prefix;
    int32_t n;
    const int32_t *worldCol;    // the table's WorldID column
};

// valid: w is a world of the executor (nothing of worldOffsets / worldCounts
// is read otherwise, and [lo, hi) is empty)
__device__ inline TeamRange teamRange(const TableHdr *hdr, uint32_t w, bool valid)
{
    TeamRange r;
    // (appends wait for the rows they take to be mapped: numRows rows are there,
    // as for digestKernel; the header's capacity word may lag behind a growth)
    int32_t n = hdr->numRows;
    n = n > 0 ? n : 0;
    int32_t prefix = hdr->sortedRows;
    if (prefix < 0 || prefix > n) {
        prefix = 0;         // whatever truncated the table: everything is "tail"
    }
    r.n = n;
    r.prefix = prefix;
    r.worldCol = (const int32_t *)hdr->columns[1];

    int32_t lo = 0, hi = 0;
    if (valid && prefix > 0) {
        const int32_t off = hdr->worldOffsets[w];
        const int32_t cnt = hdr->worldCounts[w];
        lo = off > 0 ? (off < prefix ? off : prefix) : 0;
        if (cnt > 0) {
            const int64_t end = (int64_t)off + cnt;
            hi = end < (int64_t)prefix ? (int32_t)end : prefix;
        }
        hi = hi > lo ? hi : lo;
    }
    r.lo = lo;
    r.hi = hi;
    return r;
}

}
}
