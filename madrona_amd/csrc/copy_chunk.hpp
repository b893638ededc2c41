// One workgroup moves one chunk of device memory: what the snapshot kernels
// (snapshot.hip) and the output rings (outputRingKernel, output_ring.hip)
// do per (segment, chunk) pair.  Device code of libmadrona_hip.so; not installed.
#pragma once
#include <cstdint>

namespace madrona {
namespace mwhip {

constexpr uint32_t kCopyThreads = 256;
constexpr uint32_t kCopyChunk = 16u << 10;      // bytes per chunk

typedef uint32_t CopyU4 __attribute__((ext_vector_type(4)));
using GlobalU4 = __attribute__((address_space(1))) CopyU4;
using GlobalU32 = __attribute__((address_space(1))) uint32_t;
using GlobalU8 = __attribute__((address_space(1))) uint8_t;

// n <= kCopyChunk bytes, the whole workgroup (kCopyThreads lanes)
__device__ inline void copyChunk(char *dst, const char *src, uint32_t n)
{
    const uint32_t tid = threadIdx.x;
    const unsigned long long both = (unsigned long long)dst | (unsigned long long)src;
    uint32_t done = 0;
    if ((both & 15ull) == 0ull) {
        // 16 bytes per lane, every load of the chunk issued before the first
        // store (which, the guards being per vector, waits for all of them)
        constexpr uint32_t kPerThread = kCopyChunk / 16u / kCopyThreads;
        const GlobalU4 *s4 = (const GlobalU4 *)(unsigned long long)src;
        GlobalU4 *d4 = (GlobalU4 *)(unsigned long long)dst;
        const uint32_t num_vec = n >> 4;
        CopyU4 v[kPerThread];
#pragma unroll
        for (uint32_t j = 0; j < kPerThread; j++) {
            const uint32_t i = j * kCopyThreads + tid;
            if (i < num_vec) v[j] = s4[i];
        }
#pragma unroll
        for (uint32_t j = 0; j < kPerThread; j++) {
            const uint32_t i = j * kCopyThreads + tid;
            if (i < num_vec) d4[i] = v[j];
        }
        done = num_vec << 4;
    } else if ((both & 3ull) == 0ull) {
        // dwords (a snapshot's header words, whose live side is a field of a
        // struct; a ring slot at an odd multiple of 4 bytes)
        const GlobalU32 *s1 = (const GlobalU32 *)(unsigned long long)src;
        GlobalU32 *d1 = (GlobalU32 *)(unsigned long long)dst;
        const uint32_t num_words = n >> 2;
        for (uint32_t i = tid; i < num_words; i += kCopyThreads) {
            d1[i] = s1[i];
        }
        done = num_words << 2;
    }
    // the odd bytes at the end (columns of 1, 2 bytes per row), or everything
    // when an address is not even dword aligned
    const GlobalU8 *s8 = (const GlobalU8 *)(unsigned long long)src;
    GlobalU8 *d8 = (GlobalU8 *)(unsigned long long)dst;
    for (uint32_t i = done + tid; i < n; i += kCopyThreads) {
        d8[i] = s8[i];
    }
}

}
}
