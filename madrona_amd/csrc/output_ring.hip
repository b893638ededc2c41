// libmadrona_hip.so -- output rings: exported tensors recorded per replay into
// device-resident rings, every ring of a graph's kind in one launch at the end
// of the replay (mwhip_set_output_ring, mwhip_output_ring_recorded,
// include/mwhip.h).  The input rings stay with the step graphs
// they open (runtime_launch.hip).
#include "exec_internal.hpp"
#include "copy_chunk.hpp"

namespace {

// every output ring of one kind (mwhip_set_output_ring), the kernel argument of
// outputRingKernel
struct OutputRingArgs {
    struct Ring {
        const char *src;
        char *ring;
        uint64_t slotBytes;
        uint32_t numSlots;
        uint32_t firstReplay;   // replays of the kind completed when the ring was set
    };
    Ring rings[MWHIP_MAX_OUTPUT_RINGS];
    uint64_t totalChunks;       // 16 KiB chunks over all rings
    uint32_t numRings;
    uint32_t counterWord;       // kStepReplayWord / kRenderReplayWord
};

// Last kernel before the health kernel of a graph whose kind has output rings
// (mwhip_set_output_ring): every ring of that kind in ONE launch.  Ring r's
// source goes to slot (replays of this kind since the ring was set) % num_slots
// of its ring; the counter is the one the input rings read (step graphs) or the
// render replays' own (render graphs), bumped by the health kernel that follows,
// so both ring kinds see the same k inside a replay.  Workgroups stride over
// the (ring, 16 KiB chunk) pairs: rings share the grid by the bytes they move.
// A slot's alignment depends on k * slot_bytes, so copyChunk picks the width
// (16 B, 4 B, 1 B) per replay, here.  One relaxed load, plain vector loads and
// stores, no LDS.  (args: by value in the kernel-argument segment, like PackArgs.)
__global__ void __launch_bounds__(kCopyThreads)
outputRingKernel(EcsState *S, OutputRingArgs args)
{
    TraceScope trace_scope(S);
    const uint32_t replay = __builtin_amdgcn_readfirstlane(
        __hip_atomic_load(S->replayCounter + args.counterWord, __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT));
    for (uint64_t work = blockIdx.x; work < args.totalChunks; work += gridDim.x) {
        // the ring this chunk belongs to (a ring has at least one chunk)
        uint32_t r = 0;
        uint64_t first = 0;
        for (;;) {
            const uint64_t chunks =
                (args.rings[r].slotBytes + kCopyChunk - 1u) / kCopyChunk;
            if (work < first + chunks || r + 1u >= args.numRings) break;
            first += chunks;
            r++;
        }
        const OutputRingArgs::Ring ring = args.rings[r];
        const uint64_t off = (work - first) * kCopyChunk;
        if (off >= ring.slotBytes) continue;    // (cannot happen: totalChunks counts them)
        const uint64_t left = ring.slotBytes - off;
        const uint32_t n = left < kCopyChunk ? (uint32_t)left : kCopyChunk;
        const uint32_t slot = (replay - ring.firstReplay) % ring.numSlots;
        copyChunk(ring.ring + (uint64_t)slot * ring.slotBytes + off,
                  ring.src + off, n);
    }
}

std::vector<ReplayExtras::OutputRing>::iterator
findOutputRing(ReplayExtras &extras, const void *src, uint32_t when)
{
    auto &rings = extras.outputRings;
    return std::find_if(rings.begin(), rings.end(),
        [src, when](const ReplayExtras::OutputRing &r) {
            return (const void *)r.src == src && r.when == when;
        });
}

int completedReplays(mwhip_exec *exec, uint32_t when, uint32_t *out)
{
    HIPCHK(hipStreamSynchronize(exec->stream));
    HIPCHK(hipMemcpy(out, exec->replaySignal +
        (when == MWHIP_RING_ON_RENDER ? kRenderReplayWord : kStepReplayWord),
        sizeof(*out), hipMemcpyDeviceToHost));
    return 0;
}

}

// Tail stage: the output rings of this graph's kind, one launch for all of
// them; none when the kind has no ring.
MWHIP_RT int outputRingStage(mwhip_exec *exec, const LaunchGraph &lg,
                             std::vector<KernelLaunch> &out)
{
    const uint32_t when = lg.isRender ? MWHIP_RING_ON_RENDER : MWHIP_RING_ON_STEP;
    OutputRingArgs args {};
    args.counterWord = lg.isRender ? kRenderReplayWord : kStepReplayWord;
    uint64_t bytes = 0;
    for (const ReplayExtras::OutputRing &r : exec->extras.outputRings) {
        if (r.when != when) continue;
        args.rings[args.numRings++] = { r.src, r.ring, r.slotBytes, r.numSlots, r.firstReplay };
        args.totalChunks += (r.slotBytes + kCopyChunk - 1) / kCopyChunk;
        bytes += r.slotBytes;
    }
    if (args.numRings == 0) return 0;

    KernelLaunch k;
    static_assert(sizeof(void *) + sizeof(OutputRingArgs) <= sizeof(k.argStorage));
    k.fn = (const void *)&outputRingKernel;
    k.grid = dim3((uint32_t)std::min<uint64_t>(args.totalChunks, 8ull * exec->numCUs), 1, 1);
    k.block = dim3(kCopyThreads, 1, 1);
    k.setArgs(exec->stateDev, args);
    k.name = "ring";
    k.role = lg.isRender ? "ring.out.render" : "ring.out";
    k.kind = MWHIP_NODE_RECYCLE;
    k.fixedBytes = 2.0 * (double)bytes;     // read + written
    out.push_back(k);
    return 0;
}

extern "C" int mwhip_set_output_ring(mwhip_exec *exec, const void *src, void *ring,
                                     uint64_t slot_bytes, uint32_t num_slots,
                                     uint32_t when)
{
    carryStale(exec);
    // (every refusal comes before anything changes)
    if (src == nullptr) {
        return fail(-2, "set_output_ring: no source");
    }
    if (when != MWHIP_RING_ON_STEP && when != MWHIP_RING_ON_RENDER) {
        return fail(-2, "set_output_ring: when = %u (MWHIP_RING_ON_STEP or "
                    "MWHIP_RING_ON_RENDER)", when);
    }
    if (ring != nullptr && (num_slots == 0 || slot_bytes == 0)) {
        return fail(-2, "set_output_ring: %llu bytes x %u slots (at least one of "
                    "each)", (unsigned long long)slot_bytes, num_slots);
    }
    if (exec == nullptr) {
        return fail(-2, "set_output_ring: no executor");
    }
    auto &rings = exec->extras.outputRings;
    const bool known = findOutputRing(exec->extras, src, when) != rings.end();
    if (ring != nullptr && !known && rings.size() >= MWHIP_MAX_OUTPUT_RINGS) {
        return fail(-2, "set_output_ring: at most %u rings",
                    (uint32_t)MWHIP_MAX_OUTPUT_RINGS);
    }
    if (ring == nullptr && !known) return 0;
    return changeReplayExtras(exec, [=](ReplayExtras &extras) {
        auto at = findOutputRing(extras, src, when);
        if (ring == nullptr) {
            extras.outputRings.erase(at);
            return 0;
        }
        // (every replay of every graph of that kind counts from here on)
        uint32_t done = 0;
        int rc = completedReplays(exec, when, &done);
        if (rc != 0) return rc;
        const ReplayExtras::OutputRing fresh {
            (const char *)src, (char *)ring, slot_bytes, num_slots, done, when };
        if (at != extras.outputRings.end()) {
            *at = fresh;
        } else {
            extras.outputRings.push_back(fresh);
        }
        return 0;
    });
}

extern "C" int mwhip_output_ring_recorded(mwhip_exec *exec, const void *src,
                                          uint32_t when, uint64_t *replays_out)
{
    if (exec == nullptr || replays_out == nullptr) {
        return fail(-2, "output_ring_recorded: no executor / no result");
    }
    auto at = findOutputRing(exec->extras, src, when);
    if (at == exec->extras.outputRings.end()) {
        return fail(-2, "output_ring_recorded: no output ring of kind %u on %p",
                    when, src);
    }
    HIPCHK(hipSetDevice(exec->cfg.gpu_id));
    uint32_t done = 0;
    int rc = completedReplays(exec, when, &done);
    if (rc != 0) return rc;
    // (the device counts in 32 bits and wraps; so does the difference)
    *replays_out = (uint32_t)(done - at->firstReplay);
    return 0;
}
