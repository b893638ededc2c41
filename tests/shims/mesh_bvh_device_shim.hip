// TEST INFRASTRUCTURE.  MeshBVH's queries on the device, one query per lane,
// over a tree the test hands in as host arrays and this shim uploads with
// uploadMeshBVH (tests/test_mesh_bvh_gpu.py).  Compiled as a simulator's
// device TU is (user prelude + force_cuda_host_device), so the code under test
// is what a ParallelFor node inlines.
#include <madrona/mwhip/user_prelude.hpp>
#pragma clang force_cuda_host_device begin
#include <madrona/mesh_bvh.hpp>
#pragma clang force_cuda_host_device end
#include <madrona/mesh_bvh_upload.hpp>

#include <hip/hip_runtime.h>
#include <cstring>

using namespace madrona;
using namespace madrona::math;

#define API extern "C" __attribute__((visibility("default")))

namespace {

struct Uploaded {
    MeshBVH dev;        // pointers into the device block
    MeshBVH *devStruct; // the struct itself on the device
    int gpu;
};

__global__ void __launch_bounds__(64) traceKernel(MeshBVH *bvh, uint32_t n, const float *origins,
                            const float *dirs, const float *t_max,
                            uint32_t *hit, float *t_hit, float *normals,
                            float *uvs, uint32_t *leaf_mat, uint32_t *material)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;

    int32_t stack[32];
    int32_t stack_size = 0;
    MeshBVH::HitInfo info {};
    bool h = bvh->traceRay(
        Vector3 { origins[3 * i], origins[3 * i + 1], origins[3 * i + 2] },
        Vector3 { dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2] },
        &info, stack, stack_size, t_max[i]);
    hit[i] = h ? 1u : 0u;
    t_hit[i] = h ? info.tHit : 0.f;
    normals[3 * i] = h ? info.normal.x : 0.f;
    normals[3 * i + 1] = h ? info.normal.y : 0.f;
    normals[3 * i + 2] = h ? info.normal.z : 0.f;
    uvs[2 * i] = h ? info.uv.x : 0.f;
    uvs[2 * i + 1] = h ? info.uv.y : 0.f;
    leaf_mat[i] = h ? info.leafMaterialIDX : 0u;
    material[i] = h ? bvh->getMaterialIDX(info) : 0u;
}

__global__ void __launch_bounds__(64) sweepKernel(MeshBVH *bvh, uint32_t n, const float *origins,
                            const float *dirs, const float *radii,
                            const float *t_max, float *t_out, float *normals)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;

    Vector3 normal { 0.f, 0.f, 0.f };
    float t = bvh->sphereCast(
        Vector3 { origins[3 * i], origins[3 * i + 1], origins[3 * i + 2] },
        Vector3 { dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2] },
        radii[i], &normal, t_max[i]);
    t_out[i] = t;
    normals[3 * i] = normal.x;
    normals[3 * i + 1] = normal.y;
    normals[3 * i + 2] = normal.z;
}

__global__ void __launch_bounds__(64) overlapKernel(MeshBVH *bvh, uint32_t n, const float *boxes,
                              uint32_t *counts, float *sums, uint32_t *hashes)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;

    AABB box {
        Vector3 { boxes[6 * i], boxes[6 * i + 1], boxes[6 * i + 2] },
        Vector3 { boxes[6 * i + 3], boxes[6 * i + 4], boxes[6 * i + 5] },
    };
    uint32_t count = 0;
    uint32_t hash = 2166136261u;
    Vector3 sum { 0.f, 0.f, 0.f };
    auto word = [&](float v) {
        hash = (hash ^ __float_as_uint(v)) * 16777619u;
    };
    bvh->findOverlaps(box, [&](Vector3 a, Vector3 b, Vector3 c) {
        count++;
        sum = sum + a; word(a.x); word(a.y); word(a.z);
        sum = sum + b; word(b.x); word(b.y); word(b.z);
        sum = sum + c; word(c.x); word(c.y); word(c.z);
    });
    counts[i] = count;
    sums[3 * i] = sum.x;
    sums[3 * i + 1] = sum.y;
    sums[3 * i + 2] = sum.z;
    hashes[i] = hash;
}

// device copies of a call's inputs and outputs; every one is checked
struct Buffers {
    static constexpr int kMax = 12;
    void *dev[kMax];
    void *host[kMax];
    uint64_t bytes[kMax];
    bool isOutput[kMax];
    int count = 0;
    bool ok = true;

    void *add(void *host_ptr, uint64_t num_bytes, bool is_output)
    {
        void *d = nullptr;
        if (count >= kMax || hipMalloc(&d, num_bytes == 0 ? 4 : num_bytes) != hipSuccess) {
            ok = false;
            return nullptr;
        }
        if (!is_output && hipMemcpy(d, host_ptr, num_bytes, hipMemcpyHostToDevice) != hipSuccess) {
            ok = false;
        }
        if (is_output && hipMemset(d, 0, num_bytes) != hipSuccess) {
            ok = false;
        }
        dev[count] = d;
        host[count] = host_ptr;
        bytes[count] = num_bytes;
        isOutput[count] = is_output;
        count++;
        return d;
    }

    int finish()
    {
        if (hipDeviceSynchronize() != hipSuccess) ok = false;
        for (int i = 0; i < count; i++) {
            if (ok && isOutput[i] &&
                    hipMemcpy(host[i], dev[i], bytes[i], hipMemcpyDeviceToHost) != hipSuccess) {
                ok = false;
            }
            (void)hipFree(dev[i]);
        }
        return ok ? 0 : -1;
    }
};

constexpr uint32_t kBlock = 64;

}

// nodes: 60 bytes each; vertices: x y z u v each, the padded tail included
// (num_verts does not count it).  Returns a handle, or nullptr.
API void *mbvh_dev_upload(int gpu_id, const void *nodes, uint32_t num_nodes,
                          const int32_t *materials, const float *vertices,
                          uint32_t num_verts, uint32_t num_leaves,
                          const float *root_aabb, int32_t material_idx)
{
    if (hipSetDevice(gpu_id) != hipSuccess) return nullptr;

    MeshBVH host {};
    host.nodes = (QBVHNode *)nodes;
    host.leafMats = (MeshBVH::LeafMaterial *)materials;
    host.vertices = (MeshBVH::BVHVertex *)vertices;
    memcpy(&host.rootAABB, root_aabb, sizeof(AABB));
    host.numNodes = num_nodes;
    host.numLeaves = num_leaves;
    host.numVerts = num_verts;
    host.materialIDX = material_idx;

    Uploaded *u = new Uploaded {};
    u->gpu = gpu_id;
    u->dev = uploadMeshBVH(gpu_id, host);
    if (u->dev.nodes == nullptr) {
        delete u;
        return nullptr;
    }
    u->devStruct = (MeshBVH *)mwhip_raw_alloc(gpu_id, sizeof(MeshBVH));
    if (u->devStruct == nullptr ||
            mwhip_raw_copy_h2d(gpu_id, u->devStruct, &u->dev, sizeof(MeshBVH)) != 0) {
        freeUploadedMeshBVH(gpu_id, u->dev);
        delete u;
        return nullptr;
    }
    return u;
}

API void mbvh_dev_free(void *handle)
{
    Uploaded *u = (Uploaded *)handle;
    if (u == nullptr) return;
    mwhip_raw_free(u->gpu, u->devStruct);
    freeUploadedMeshBVH(u->gpu, u->dev);
    delete u;
}

// The uploaded block: offsets[3] of the three arrays from the block's base
// (= nodes), sizes[2] = { vertex bytes with the tail, block bytes }, and the
// whole block copied to block_out (if not null; sizes[1] bytes).
API int mbvh_dev_block(void *handle, uint64_t *offsets, uint64_t *sizes,
                       void *block_out)
{
    Uploaded *u = (Uploaded *)handle;
    MeshBVHUploadLayout l = meshBVHUploadLayout(u->dev);
    char *base = (char *)u->dev.nodes;
    offsets[0] = 0;
    offsets[1] = (uint64_t)((char *)u->dev.leafMats - base);
    offsets[2] = (uint64_t)((char *)u->dev.vertices - base);
    sizes[0] = l.numVertexBytes;
    sizes[1] = l.numBytes;
    if (block_out == nullptr) return 0;
    return mwhip_raw_copy_d2h(u->gpu, block_out, base, l.numBytes);
}

API int mbvh_dev_trace(void *handle, uint32_t n, float *origins, float *dirs,
                       float *t_max, uint32_t *hit, float *t_hit,
                       float *normals, float *uvs, uint32_t *leaf_mat,
                       uint32_t *material)
{
    Uploaded *u = (Uploaded *)handle;
    Buffers b;
    auto *d_o = (float *)b.add(origins, 12ull * n, false);
    auto *d_d = (float *)b.add(dirs, 12ull * n, false);
    auto *d_tm = (float *)b.add(t_max, 4ull * n, false);
    auto *d_hit = (uint32_t *)b.add(hit, 4ull * n, true);
    auto *d_t = (float *)b.add(t_hit, 4ull * n, true);
    auto *d_n = (float *)b.add(normals, 12ull * n, true);
    auto *d_uv = (float *)b.add(uvs, 8ull * n, true);
    auto *d_lm = (uint32_t *)b.add(leaf_mat, 4ull * n, true);
    auto *d_m = (uint32_t *)b.add(material, 4ull * n, true);
    if (b.ok) {
        traceKernel<<<(n + kBlock - 1) / kBlock, kBlock>>>(u->devStruct, n,
            d_o, d_d, d_tm, d_hit, d_t, d_n, d_uv, d_lm, d_m);
        if (hipGetLastError() != hipSuccess) b.ok = false;
    }
    return b.finish();
}

API int mbvh_dev_sweep(void *handle, uint32_t n, float *origins, float *dirs,
                       float *radii, float *t_max, float *t_out,
                       float *normals)
{
    Uploaded *u = (Uploaded *)handle;
    Buffers b;
    auto *d_o = (float *)b.add(origins, 12ull * n, false);
    auto *d_d = (float *)b.add(dirs, 12ull * n, false);
    auto *d_r = (float *)b.add(radii, 4ull * n, false);
    auto *d_tm = (float *)b.add(t_max, 4ull * n, false);
    auto *d_t = (float *)b.add(t_out, 4ull * n, true);
    auto *d_n = (float *)b.add(normals, 12ull * n, true);
    if (b.ok) {
        sweepKernel<<<(n + kBlock - 1) / kBlock, kBlock>>>(u->devStruct, n,
            d_o, d_d, d_r, d_tm, d_t, d_n);
        if (hipGetLastError() != hipSuccess) b.ok = false;
    }
    return b.finish();
}

API int mbvh_dev_overlap(void *handle, uint32_t n, float *boxes,
                         uint32_t *counts, float *sums, uint32_t *hashes)
{
    Uploaded *u = (Uploaded *)handle;
    Buffers b;
    auto *d_b = (float *)b.add(boxes, 24ull * n, false);
    auto *d_c = (uint32_t *)b.add(counts, 4ull * n, true);
    auto *d_s = (float *)b.add(sums, 12ull * n, true);
    auto *d_h = (uint32_t *)b.add(hashes, 4ull * n, true);
    if (b.ok) {
        overlapKernel<<<(n + kBlock - 1) / kBlock, kBlock>>>(u->devStruct, n,
            d_b, d_c, d_s, d_h);
        if (hipGetLastError() != hipSuccess) b.ok = false;
    }
    return b.finish();
}
