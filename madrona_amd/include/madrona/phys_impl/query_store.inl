// What the kernels that run the step's narrowphase from outside the step store
// of a manifold (shape_query.inl; contact_query.inl keeps its own copy for now
// and could include this instead): normal and points of a ContactConstraint in
// the layout of mwhip_contacts_* / mwhip_shapes_*, and the zeros of an unused
// slot.  Included by physics.inl inside madrona::phys::kernels.

namespace queryst {

// normal[slot][3], points[slot][4][4]; point slots >= numPoints are zero (the
// step leaves what it likes behind numPoints)
__device__ inline void storeManifold(int32_t *num_points, float *normal, float *points,
                                     uint64_t slot, const ContactConstraint &contact)
{
    num_points[slot] = contact.numPoints;
    float *n = normal + slot * 3ull;
    n[0] = contact.normal.x;
    n[1] = contact.normal.y;
    n[2] = contact.normal.z;
    float *p = points + slot * 16ull;
#pragma unroll
    for (int32_t i = 0; i < 4; i++) {
        const bool used = i < contact.numPoints;
        p[i * 4 + 0] = used ? contact.points[i].x : 0.f;
        p[i * 4 + 1] = used ? contact.points[i].y : 0.f;
        p[i * 4 + 2] = used ? contact.points[i].z : 0.f;
        p[i * 4 + 3] = used ? contact.points[i].w : 0.f;
    }
}

__device__ inline void storeNoManifold(int32_t *num_points, float *normal, float *points,
                                       uint64_t slot)
{
    num_points[slot] = 0;
    float *n = normal + slot * 3ull;
    n[0] = n[1] = n[2] = 0.f;
    float *p = points + slot * 16ull;
#pragma unroll
    for (int32_t i = 0; i < 16; i++) {
        p[i] = 0.f;
    }
}

}
