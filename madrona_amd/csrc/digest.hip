// libmadrona_hip.so -- state digests: a 64-bit hash per world of a chosen set of
// columns, computed on the device (mwhip_digest_*, include/mwhip.h).
//
// A digest owns a device-resident PLAN -- per group (the listed columns of one
// table) the table header, the group's tag and its column range; per column the
// header slot its base address is read from (the sort swaps a column with its
// twin), the cell bytes and the column's tag -- and a buffer D[groups][worlds].
// Row counts and column bases are read on the device when the kernel runs: no
// host round trip, and a plan made before a table grew is still right after.
//   digestZero     clears D (a memset where nothing is captured, a kernel node
//                  of its own in a step graph: the launch graphs hold kernel
//                  nodes only)
//   digestKernel   workgroups of 256 stride over the (group, block of 256 rows)
//                  pairs, one lane per row: hash the row's listed cells in plan
//                  order, sum the hashes of each run of equal world ids inside
//                  the wavefront (one inclusive scan; sums are modulo 2^64, so a
//                  run's sum is a difference of two prefix sums), then ONE
//                  no-return atomic add per (wavefront, distinct world) into D.
// Integer adds commute: D is the same whatever order the waves arrive in.  No
// spin-waits, no cross-workgroup protocol, no LDS.
#include "exec_internal.hpp"

namespace {

constexpr uint32_t kDigestThreads = 256;
constexpr uint64_t kDigestK1 = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kDigestK2 = 0xBF58476D1CE4E5B9ull;
constexpr uint64_t kDigestK3 = 0x94D049BB133111EBull;

struct DigestPlanColumn {
    void *const *slot;      // &hdr->columns[c] on the device
    uint32_t cellBytes;
    uint32_t tag;           // position in the plan
};

struct DigestPlanGroup {
    const TableHdr *hdr;    // on the device
    uint32_t tag;           // plan position of the group's first column
    uint32_t firstColumn;   // into the plan's (group-ordered) columns
    uint32_t numColumns;
    uint32_t rowBytes;      // of the listed cells
};

// head of the device-resident plan; behind it
//   DigestPlanGroup  groups[numGroups]
//   DigestPlanColumn columns[numColumns]
struct DigestPlan {
    uint32_t numGroups;
    uint32_t numColumns;
    uint32_t numWorlds;
    uint32_t pad_;
};

__host__ __device__ inline DigestPlanGroup *planGroups(DigestPlan *plan)
{
    return (DigestPlanGroup *)(plan + 1);
}

__host__ __device__ inline DigestPlanColumn *planColumns(DigestPlan *plan, uint32_t num_groups)
{
    return (DigestPlanColumn *)(planGroups(plan) + num_groups);
}

__device__ inline uint64_t digestFin(uint64_t x)
{
    x ^= x >> 30; x *= kDigestK2;
    x ^= x >> 27; x *= kDigestK3;
    x ^= x >> 31;
    return x;
}

__device__ inline uint64_t digestAbsorb(uint64_t h, uint64_t v)
{
    h = (h ^ v) * kDigestK1;
    return h ^ (h >> 32);
}

// the little-endian dwords of one cell, in order, zero-padded at the end; read
// with the widest load the cell's size and its column's alignment allow
__device__ inline uint64_t digestCell(uint64_t h, const char *cell, uint32_t bytes,
                                      bool base16)
{
    if (bytes % 16u == 0u && base16) {
        const uint4 *p = (const uint4 *)cell;
        for (uint32_t i = 0; i < bytes / 16u; i++) {
            const uint4 v = p[i];
            h = digestAbsorb(h, v.x);
            h = digestAbsorb(h, v.y);
            h = digestAbsorb(h, v.z);
            h = digestAbsorb(h, v.w);
        }
    } else if (bytes % 8u == 0u && base16) {
        const uint2 *p = (const uint2 *)cell;
        for (uint32_t i = 0; i < bytes / 8u; i++) {
            const uint2 v = p[i];
            h = digestAbsorb(h, v.x);
            h = digestAbsorb(h, v.y);
        }
    } else if (bytes % 4u == 0u && base16) {
        const uint32_t *p = (const uint32_t *)cell;
        for (uint32_t i = 0; i < bytes / 4u; i++) {
            h = digestAbsorb(h, p[i]);
        }
    } else if (bytes % 2u == 0u && base16) {
        const uint16_t *p = (const uint16_t *)cell;
        const uint32_t halves = bytes / 2u;
        for (uint32_t i = 0; i < halves; i += 2u) {
            uint32_t v = p[i];
            if (i + 1u < halves) v |= (uint32_t)p[i + 1u] << 16;
            h = digestAbsorb(h, v);
        }
    } else {
        const uint8_t *p = (const uint8_t *)cell;
        for (uint32_t i = 0; i < bytes; i += 4u) {
            uint32_t v = 0;
            for (uint32_t b = 0; b < 4u && i + b < bytes; b++) {
                v |= (uint32_t)p[i + b] << (8u * b);
            }
            h = digestAbsorb(h, v);
        }
    }
    return h;
}

__device__ inline uint64_t shflU64(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int32_t)(uint32_t)v, src, 64);
    const uint32_t hi = (uint32_t)__shfl((int32_t)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ inline uint64_t shflUpU64(uint64_t v, uint32_t delta)
{
    const uint32_t lo = (uint32_t)__shfl_up((int32_t)(uint32_t)v, delta, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int32_t)(uint32_t)(v >> 32), delta, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ inline void digestAdd(unsigned long long *addr, uint64_t v)
{
    // (result unused: a no-return atomic)
    (void)__hip_atomic_fetch_add(addr, (unsigned long long)v, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kDigestThreads)
digestZero(unsigned long long *out, uint32_t count)
{
    for (uint32_t i = blockIdx.x * kDigestThreads + threadIdx.x; i < count;
         i += gridDim.x * kDigestThreads) {
        out[i] = 0ull;
    }
}

// out: D[numGroups][numWorlds], and behind it one word that counts the bytes of
// the cells hashed (mwhip_profile's algo_bytes)
__global__ void __launch_bounds__(kDigestThreads)
digestKernel(DigestPlan *plan, unsigned long long *out)
{
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t num_groups = plan->numGroups;
    const int32_t num_worlds = (int32_t)plan->numWorlds;
    const DigestPlanGroup *groups = planGroups(plan);
    const DigestPlanColumn *columns = planColumns(plan, num_groups);
    const uint32_t G = gridDim.x;

    uint64_t cell_bytes = 0;    // hashed by this wavefront (uniform)
    uint32_t start = 0;         // work items of the groups before this one
    for (uint32_t g = 0; g < num_groups; g++) {
        const DigestPlanGroup grp = groups[g];
        const int32_t rows_now = grp.hdr->numRows;
        const uint32_t n = (uint32_t)(rows_now > 0 ? rows_now : 0);
        const uint32_t blocks = (n + kDigestThreads - 1u) / kDigestThreads;
        // this workgroup's first block of the group: work items are dealt
        // round robin over the whole (group, block) sequence
        uint32_t b = (blockIdx.x + G - start % G) % G;
        start += blocks;
        if (b >= blocks) continue;

        const int32_t *world_col = (const int32_t *)grp.hdr->columns[1];
        unsigned long long *D = out + (uint64_t)g * (uint32_t)num_worlds;
        for (; b < blocks; b += G) {
            const uint32_t row = b * kDigestThreads + threadIdx.x;
            int32_t world = -1;
            if (row < n) world = world_col[row];
            // (never index D with an id that was not checked)
            const bool live = world >= 0 && world < num_worlds;
            uint64_t h = 0;
            if (live) {
                h = digestFin((uint64_t)grp.tag + kDigestK1);
                for (uint32_t c = 0; c < grp.numColumns; c++) {
                    const DigestPlanColumn col = columns[grp.firstColumn + c];
                    const char *base = (const char *)*col.slot;
                    h = digestAbsorb(h, col.tag);
                    h = digestCell(h, base + (uint64_t)row * col.cellBytes, col.cellBytes,
                                   ((uint64_t)base & 15ull) == 0ull);
                }
                h = digestFin(h);
            }
            const unsigned long long live_mask = __ballot(live);
            if (live_mask == 0ull) continue;
            cell_bytes += (uint64_t)__builtin_popcountll(live_mask) * grp.rowBytes;

            // runs of equal world ids (rows that add nothing are world -1 and
            // form runs of their own)
            const int32_t key = live ? world : -1;
            const int32_t prev_key = __shfl_up(key, 1u, 64);
            const bool head = lane == 0u || key != prev_key;
            const unsigned long long heads = __ballot(head);
            // inclusive scan over the wavefront, modulo 2^64
            uint64_t prefix = h;
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const uint64_t below = shflUpU64(prefix, d);
                if (lane >= d) prefix += below;
            }
            // the run's sum, in its last lane: prefix[last] - prefix[first - 1]
            const unsigned long long upto = heads & (~0ull >> (63u - lane));
            const int first = 63 - __builtin_clzll(upto);    // (bit 0 is always set)
            const uint64_t before = shflU64(prefix, first > 0 ? first - 1 : 0);
            const uint64_t run_sum = prefix - (first > 0 ? before : 0ull);
            const bool tail = live && (lane == 63u || ((heads >> (lane + 1u)) & 1ull) != 0ull);
            unsigned long long tails = __ballot(tail);

            // Sorted rows without holes: every run is another world, its last
            // lane adds.  Otherwise (an unsorted tail, rows destroyed in
            // place) a world may own several runs: their sums are merged
            // first, so that a wavefront never adds twice to one address.
            const bool descends = live && lane != 0u && prev_key > key;
            const unsigned long long valid_mask = __ballot(row < n);
            if (live_mask == valid_mask && __ballot(descends) == 0ull) {
                if (tail) digestAdd(D + world, run_sum);
                continue;
            }
            while (tails != 0ull) {
                const int leader = __builtin_ctzll(tails);
                const int32_t lead_world = __shfl(world, leader, 64);
                const unsigned long long same = __ballot(tail && world == lead_world);
                uint64_t sum = 0;
                for (unsigned long long rest = same; rest != 0ull; rest &= rest - 1ull) {
                    sum += shflU64(run_sum, __builtin_ctzll(rest));
                }
                if ((int)lane == leader) digestAdd(D + world, sum);
                tails &= ~same;
            }
        }
    }
    if (lane == 0u && cell_bytes != 0ull) {
        digestAdd(out + (uint64_t)num_groups * (uint32_t)num_worlds, cell_bytes);
    }
}

}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct mwhip_digest_rec {
    uint64_t handle = 0;
    uint32_t numGroups = 0;
    uint32_t numWorlds = 0;
    std::vector<uint32_t> groupArchetype;
    std::vector<uint32_t> groupTag;
    DigestPlan *planDev = nullptr;
    unsigned long long *outDev = nullptr;   // D, then the cell-byte counter

    ~mwhip_digest_rec()
    {
        if (planDev != nullptr) (void)hipFree(planDev);
        if (outDev != nullptr) (void)hipFree(outDev);
    }
};

namespace {

mwhip_digest_rec *findDigest(mwhip_exec *exec, uint64_t handle)
{
    return findObject(exec != nullptr ? &exec->digests : nullptr, handle);
}

uint32_t digestWords(const mwhip_digest_rec &dig)
{
    return dig.numGroups * dig.numWorlds + 1u;
}

int queueDigest(mwhip_exec *exec, mwhip_digest_rec &dig)
{
    HIPCHK(hipMemsetAsync(dig.outDev, 0, (size_t)digestWords(dig) * 8u, exec->stream));
    hipLaunchKernelGGL(digestKernel, dim3(std::max(exec->numCUs, 1u) * 8u),
                       dim3(kDigestThreads), 0, exec->stream, dig.planDev, dig.outDev);
    HIPCHK(hipGetLastError());
    return 0;
}

int computeDigest(mwhip_exec *exec, uint64_t digest, bool wait)
{
    mwhip_digest_rec *dig = findDigest(exec, digest);
    if (dig == nullptr) return unknownObject("digest", digest);
    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    return finishQueued(exec, queueDigest(exec, *dig), wait);
}

// Bytes of the cells the step digest's last run hashed (KernelLaunch::measuredBytes).
int stepDigestCellBytes(mwhip_exec *exec, double *out)
{
    *out = 0;
    mwhip_digest_rec *dig = findDigest(exec, exec->extras.stepDigest);
    if (dig == nullptr) return 0;
    unsigned long long bytes = 0;
    HIPCHK(hipMemcpy(&bytes, dig->outDev + (size_t)dig->numGroups * dig->numWorlds,
                     sizeof(bytes), hipMemcpyDeviceToHost));
    *out = (double)bytes;
    return 0;
}

}

// Tail stage: the two launches that recompute the step digest inside a step
// replay; none when no step digest is set.
MWHIP_RT int stepDigestStage(mwhip_exec *exec, const LaunchGraph &lg,
                             std::vector<KernelLaunch> &out)
{
    mwhip_digest_rec *dig = findDigest(exec, exec->extras.stepDigest);
    if (lg.isRender || dig == nullptr) return 0;
    const uint32_t words = digestWords(*dig);

    KernelLaunch zero;
    zero.fn = (const void *)&digestZero;
    zero.grid = dim3(std::min((words + kDigestThreads - 1u) / kDigestThreads,
                              std::max(exec->numCUs, 1u) * 8u), 1, 1);
    zero.block = dim3(kDigestThreads, 1, 1);
    zero.setArgs(dig->outDev, words);
    zero.name = "digest";
    zero.role = "digest.zero";
    zero.kind = MWHIP_NODE_RECYCLE;
    zero.fixedBytes = (double)words * 8.0;
    out.push_back(zero);

    KernelLaunch k;
    k.fn = (const void *)&digestKernel;
    k.grid = dim3(std::max(exec->numCUs, 1u) * 8u, 1, 1);
    k.block = dim3(kDigestThreads, 1, 1);
    k.setArgs(dig->planDev, dig->outDev);
    k.name = "digest";
    k.role = "digest";
    k.kind = MWHIP_NODE_RECYCLE;
    // the cells of the live rows it hashed, counted by the kernel
    k.measuredBytes = &stepDigestCellBytes;
    out.push_back(k);
    return 0;
}

extern "C" int mwhip_digest_create(mwhip_exec *exec, const mwhip_digest_column *cols,
                                   uint32_t n, uint64_t *digest_out)
{
    carryStale(exec);
    // (every refusal comes before anything is allocated)
    if (exec == nullptr || !exec->stateBuilt || digest_out == nullptr) {
        return fail(-2, "digest_create: no executor state");
    }
    if (n == 0 || cols == nullptr) {
        return fail(-2, "digest_create: no columns (n == 0)");
    }
    if (n > MWHIP_DIGEST_MAX_COLUMNS) {
        return fail(-2, "digest_create: %u columns (at most %u)", n,
                    (uint32_t)MWHIP_DIGEST_MAX_COLUMNS);
    }
    std::vector<ResolvedColumn> resolved;
    int rc = resolveColumns(exec, "digest_create", cols, n, resolved);
    if (rc != 0) return rc;
    struct HostGroup {
        uint32_t archetype, tag, rowBytes;
        std::vector<DigestPlanColumn> columns;
    };
    std::vector<HostGroup> groups;
    const EcsState &hs = exec->hostState;
    for (uint32_t p = 0; p < n; p++) {
        const uint32_t a = cols[p].archetype_id;
        auto at = std::find_if(groups.begin(), groups.end(),
            [a](const HostGroup &g) { return g.archetype == a; });
        if (at == groups.end()) {
            if (groups.size() >= MWHIP_DIGEST_MAX_GROUPS) {
                return fail(-2, "digest_create: more than %u groups (tables)",
                            (uint32_t)MWHIP_DIGEST_MAX_GROUPS);
            }
            groups.push_back({ a, p, 0u, {} });
            at = groups.end() - 1;
        }
        at->columns.push_back({ resolved[p].slot, resolved[p].cellBytes, p });
        at->rowBytes += resolved[p].cellBytes;
    }

    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    std::unique_ptr<mwhip_digest_rec> dig(new mwhip_digest_rec {});
    dig->numGroups = (uint32_t)groups.size();
    dig->numWorlds = exec->cfg.num_worlds;

    std::vector<char> meta(sizeof(DigestPlan) + groups.size() * sizeof(DigestPlanGroup) +
                           (size_t)n * sizeof(DigestPlanColumn), 0);
    DigestPlan *plan = (DigestPlan *)meta.data();
    plan->numGroups = dig->numGroups;
    plan->numColumns = n;
    plan->numWorlds = dig->numWorlds;
    DigestPlanGroup *plan_groups = planGroups(plan);
    DigestPlanColumn *plan_columns = planColumns(plan, dig->numGroups);
    uint32_t first = 0;
    for (size_t g = 0; g < groups.size(); g++) {
        const HostGroup &hg = groups[g];
        plan_groups[g] = { hs.tables + hg.archetype, hg.tag, first,
                           (uint32_t)hg.columns.size(), hg.rowBytes };
        memcpy(plan_columns + first, hg.columns.data(),
               hg.columns.size() * sizeof(DigestPlanColumn));
        first += (uint32_t)hg.columns.size();
        dig->groupArchetype.push_back(hg.archetype);
        dig->groupTag.push_back(hg.tag);
    }

    if (hipMalloc((void **)&dig->planDev, meta.size()) != hipSuccess ||
            hipMalloc((void **)&dig->outDev, (size_t)digestWords(*dig) * 8u) != hipSuccess ||
            hipMemcpy(dig->planDev, meta.data(), meta.size(),
                      hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(dig->outDev, 0, (size_t)digestWords(*dig) * 8u) != hipSuccess) {
        return CREATE_FAILED(dig, "digest_create: no device memory for the plan and "
                             "%u x %u words", (uint32_t)groups.size(), exec->cfg.num_worlds);
    }
    *digest_out = exec->digests.insert(std::move(dig));
    return 0;
}

extern "C" int mwhip_set_step_digest(mwhip_exec *exec, uint64_t digest)
{
    carryStale(exec);
    if (digest != 0 && findDigest(exec, digest) == nullptr) {
        return unknownObject("digest", digest);
    }
    if (exec == nullptr) return fail(-2, "set_step_digest: no executor");
    if (exec->extras.stepDigest == digest) return 0;
    return changeReplayExtras(exec, [digest](ReplayExtras &extras) {
        extras.stepDigest = digest;
        return 0;
    });
}

extern "C" void mwhip_digest_destroy(mwhip_exec *exec, uint64_t digest)
{
    carryStale(exec);
    if (findDigest(exec, digest) == nullptr) return;
    (void)hipSetDevice(exec->cfg.gpu_id);
    // (the step graphs must stop naming its buffers before they go; if they
    // could not be rebuilt without it, it stays until mwhip_destroy)
    if (exec->extras.stepDigest == digest && mwhip_set_step_digest(exec, 0) != 0) return;
    (void)hipStreamSynchronize(exec->stream);
    exec->digests.erase(digest);
}

extern "C" int mwhip_digest_compute(mwhip_exec *exec, uint64_t digest)
{
    carryStale(exec);
    return computeDigest(exec, digest, true);
}

extern "C" int mwhip_digest_compute_async(mwhip_exec *exec, uint64_t digest)
{
    carryStale(exec);
    return computeDigest(exec, digest, false);
}

extern "C" void *mwhip_digest_buffer(mwhip_exec *exec, uint64_t digest,
                                     uint32_t *groups_out, uint32_t *worlds_out)
{
    mwhip_digest_rec *dig = findDigest(exec, digest);
    if (dig == nullptr) {
        (void)unknownObject("digest", digest);
        return nullptr;
    }
    if (groups_out != nullptr) *groups_out = dig->numGroups;
    if (worlds_out != nullptr) *worlds_out = dig->numWorlds;
    return dig->outDev;
}

extern "C" int mwhip_digest_group(mwhip_exec *exec, uint64_t digest, uint32_t group,
                                  uint32_t *archetype_out, uint32_t *tag_out)
{
    mwhip_digest_rec *dig = findDigest(exec, digest);
    if (dig == nullptr) return unknownObject("digest", digest);
    if (group >= dig->numGroups) {
        return fail(-2, "digest_group: group %u of %u", group, dig->numGroups);
    }
    if (archetype_out != nullptr) *archetype_out = dig->groupArchetype[group];
    if (tag_out != nullptr) *tag_out = dig->groupTag[group];
    return 0;
}
