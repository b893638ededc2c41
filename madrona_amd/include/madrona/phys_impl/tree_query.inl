// What ray queries (ray_query.inl) and box queries (box_query.inl) share on the
// device.  Included once by physics.inl inside madrona::phys::kernels, ahead of
// both.

namespace treeq {

__device__ inline bool finiteBits(float v)
{
    return (__builtin_bit_cast(uint32_t, v) & 0x7F800000u) != 0x7F800000u;
}

__device__ inline bool nanBits(float v)
{
    return (__builtin_bit_cast(uint32_t, v) & 0x7FFFFFFFu) > 0x7F800000u;
}

enum class HeadCode : int32_t { Ok, BadWorld, Skipped, BadPoint };

struct GroupHead {
    HeadCode code;
    int32_t world;
    float x, y, z;
};

// World, count and point (a fan's origin, a bundle's centre) of group `group`,
// read and checked in that order by ONE lane; nothing behind a check that
// failed is read.  groups_per_world > 0: world = group / groups_per_world, and
// with a count source the groups at or past their world's count are skipped.
__device__ inline GroupHead readGroupHead(const char *world_src, uint32_t world_stride,
                                          const char *count_src, uint32_t count_stride,
                                          const char *point_src, uint32_t point_stride,
                                          uint32_t groups_per_world, uint32_t group,
                                          const EcsState *S)
{
    GroupHead head { HeadCode::Ok, 0, 0.f, 0.f, 0.f };
    if (groups_per_world != 0u) {
        head.world = (int32_t)(group / groups_per_world);
    } else {
        head.world = *(const int32_t *)(world_src + (uint64_t)group * world_stride);
    }
    if (head.world < 0 || head.world >= S->numWorlds) {
        head.code = HeadCode::BadWorld;
    } else if (count_src != nullptr && groups_per_world != 0u &&
               (int32_t)(group % groups_per_world) >=
                   *(const int32_t *)(count_src +
                                      (uint64_t)(uint32_t)head.world * count_stride)) {
        head.code = HeadCode::Skipped;
    } else {
        const float *p = (const float *)(point_src + (uint64_t)group * point_stride);
        head.x = p[0];
        head.y = p[1];
        head.z = p[2];
        if (!finiteBits(head.x) || !finiteBits(head.y) || !finiteBits(head.z)) {
            head.code = HeadCode::BadPoint;
        }
    }
    return head;
}

}
