// What ray queries (ray_query.hip) and box queries (box_query.hip) share on the
// host: both are GROUPS -- fans of rays, bundles of boxes -- that share a world
// and a point (origin, centre), tested through the worlds' broadphase BVHs by a
// kernel of the simulator's code object.  World, count and point are each an
// owned buffer or a mwhip_ray_source of the caller's, or, for the world, the
// rule world = group / groups_per_world.  Here, once: the record, its one
// allocation, the refusals about the sources, where the kernel reads an item,
// the _buffer accessor.  Contact queries (contact_query.hip) and shape queries
// (shape_query.hip), which go through no tree, use the record, the allocation, the item source and the accessor.
// Host code only; included behind exec_internal.hpp.
// Not installed.
#pragma once
#include "exec_internal.hpp"

// A query's record: one device allocation (bufDev) that holds its NUM_BUFS
// buffers, 256-byte aligned each, and the device-resident plan.
template <typename Plan, uint32_t NUM_BUFS>
struct TreeQueryRec {
    uint64_t handle = 0;
    uint32_t items = 0;         // wavefront work items
    char *bufs[NUM_BUFS] = {};  // into bufDev; null: not owned
    uint64_t bytes[NUM_BUFS] = {};
    Plan *planDev = nullptr;
    char *bufDev = nullptr;

    ~TreeQueryRec()
    {
        if (planDev != nullptr) (void)hipFree(planDev);
        if (bufDev != nullptr) (void)hipFree(bufDev);
    }
};

// Allocates the plan and ONE zeroed allocation for the buffers rec.bytes[]
// sizes, and points rec.bufs[] into it (null where bytes is 0).  false: no
// device memory (the record frees what it got).  *total_out: the allocation's
// bytes, for the message.
template <typename Plan, uint32_t NUM_BUFS>
inline bool allocQueryBuffers(TreeQueryRec<Plan, NUM_BUFS> &rec, uint64_t *total_out)
{
    uint64_t offsets[NUM_BUFS];
    uint64_t total = 0;
    for (uint32_t b = 0; b < NUM_BUFS; b++) {
        offsets[b] = total;
        total += (rec.bytes[b] + 255ull) & ~255ull;
    }
    *total_out = total;
    if (hipMalloc((void **)&rec.bufDev, total) != hipSuccess ||
            hipMalloc((void **)&rec.planDev, sizeof(Plan)) != hipSuccess ||
            hipMemset(rec.bufDev, 0, total) != hipSuccess) {
        return false;
    }
    for (uint32_t b = 0; b < NUM_BUFS; b++) {
        if (rec.bytes[b] != 0ull) rec.bufs[b] = rec.bufDev + offsets[b];
    }
    return true;
}

// what `who` (rays_create, boxes_create) refuses about a source of `item_bytes`
// per record
inline int checkItemSource(const char *who, const char *name, const mwhip_ray_source &source,
                           uint32_t item_bytes)
{
    if (((uint64_t)source.src & 3ull) != 0ull || source.record_bytes % 4u != 0u ||
            source.first_byte % 4u != 0u) {
        return fail(-2, "%s: %s: src %p, record_bytes %u and first_byte %u must be "
                    "multiples of 4", who, name, source.src, source.record_bytes,
                    source.first_byte);
    }
    if ((uint64_t)source.first_byte + item_bytes > (uint64_t)source.record_bytes) {
        return fail(-2, "%s: %s: %u bytes from byte %u do not fit a record of %u bytes", who,
                    name, item_bytes, source.first_byte, source.record_bytes);
    }
    return 0;
}

// ... and about the three of a create, in the order world, count, point.
// `rule`: the descriptor's groups-per-world field by name, by_rule: it is set.
inline int checkGroupSources(const char *who, bool by_rule, const char *rule,
                             const mwhip_ray_source &world, const mwhip_ray_source &count,
                             const char *point_name, const mwhip_ray_source &point)
{
    int rc = 0;
    if (!by_rule && world.src != nullptr) rc = checkItemSource(who, "world", world, 4u);
    if (rc == 0 && count.src != nullptr) {
        if (!by_rule) return fail(-2, "%s: a count source needs %s > 0", who, rule);
        rc = checkItemSource(who, "count", count, 4u);
    }
    if (rc == 0 && point.src != nullptr) rc = checkItemSource(who, point_name, point, 12u);
    return rc;
}

// Where the kernel reads an item: in the query's own buffer `own_buf` (records
// of own_stride bytes) if it owns one (`own`), else in the caller's source, else
// (no source given: a count) nowhere.  (A world that a rule replaces is not
// resolved at all: the descriptor's source is ignored then.)
inline void resolveItemSource(bool own, const char *own_buf, uint32_t own_stride,
                              const mwhip_ray_source &source, const char **src, uint32_t *stride)
{
    if (own) {
        *src = own_buf;
        *stride = own_stride;
    } else if (source.src != nullptr) {
        *src = (const char *)source.src + source.first_byte;
        *stride = source.record_bytes;
    }
}

// mwhip_rays_buffer / mwhip_boxes_buffer: `rec` is what the lookup found,
// `entry` the entry point and `rule` the descriptor's field, for the messages.
template <typename Plan, uint32_t NUM_BUFS>
inline void *queryBuffer(TreeQueryRec<Plan, NUM_BUFS> *rec, const char *kind, uint64_t handle,
                         const char *entry, const char *rule, uint32_t which,
                         uint64_t *bytes_out)
{
    if (rec == nullptr) {
        (void)unknownObject(kind, handle);
        return nullptr;
    }
    if (which >= NUM_BUFS) {
        (void)fail(-2, "%s: buffer %u of %u", entry, which, NUM_BUFS);
        return nullptr;
    }
    if (rec->bufs[which] == nullptr) {
        (void)fail(-2, "%s: buffer %u is not owned (a source or %s was given)", entry, which,
                   rule);
        return nullptr;
    }
    if (bytes_out != nullptr) *bytes_out = rec->bytes[which];
    return rec->bufs[which];
}
