// <madrona/math.hpp> compiled for the host behind a C ABI: Vector3::normalize
// and Quat::rotateVec, the two functions the simulators' ray systems build
// their directions with (fanDirection of sims/broadphase_only, lidarSystem of
// sims/escape_room_phys).  tests/test_ray_directions.py pins the float32
// restatement of madrona_amd/ray_ref.py against them bit for bit.
#include <madrona/math.hpp>

#include <cstdint>

using madrona::math::Quat;
using madrona::math::Vector3;

#define RAYDIR_API extern "C" __attribute__((visibility("default")))

// out[i] = in[i].normalize()
RAYDIR_API void raydir_normalize(const float *in, float *out, int32_t n)
{
    for (int32_t i = 0; i < n; i++) {
        const Vector3 v = Vector3 { in[3 * i], in[3 * i + 1], in[3 * i + 2] }.normalize();
        out[3 * i] = v.x;
        out[3 * i + 1] = v.y;
        out[3 * i + 2] = v.z;
    }
}

// out[q][i] = quats[q].rotateVec(vecs[i]).normalize(); quats are (w, x, y, z)
RAYDIR_API void raydir_rotate_normalize(const float *quats, int32_t num_quats,
                                        const float *vecs, int32_t num_vecs, float *out)
{
    for (int32_t q = 0; q < num_quats; q++) {
        const Quat rot { quats[4 * q], quats[4 * q + 1], quats[4 * q + 2], quats[4 * q + 3] };
        for (int32_t i = 0; i < num_vecs; i++) {
            const Vector3 v = rot.rotateVec(
                Vector3 { vecs[3 * i], vecs[3 * i + 1], vecs[3 * i + 2] }).normalize();
            float *o = out + 3 * ((int64_t)q * num_vecs + i);
            o[0] = v.x;
            o[1] = v.y;
            o[2] = v.z;
        }
    }
}
