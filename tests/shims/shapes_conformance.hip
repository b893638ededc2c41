// TEST INFRASTRUCTURE.  The shape query API conformance check (see
// shapes_conformance.inl) once more as a HIP translation unit compiled for
// gfx950, wrapped like a simulator's (user prelude, then the
// force_cuda_host_device pragma): the executor header where device code is
// compiled too.
#include <madrona/mwhip/user_prelude.hpp>
#pragma clang force_cuda_host_device begin
#include <madrona/mw_gpu.hpp>
#pragma clang force_cuda_host_device end

// (host functions, as the Manager's are)
#define SHAPESCONF_NAME shapesconf_hip
#include "shapes_conformance.inl"

namespace {

// (makes this a translation unit with a gfx950 code object)
__global__ void shapesconfTouch(uint64_t *out, uint64_t value)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        *out = value;
    }
}

}

extern "C" SHAPESCONF_API const void *shapesconf_hip_kernel()
{
    return (const void *)shapesconfTouch;
}
