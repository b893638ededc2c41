// The render side of a simulator's manager: the bridge the reference's CPU-mode
// render-prep systems append their records to (cpu_render_bridge.hpp; the HIP
// backend has none: there the render entities' rows are the records), the one
// C entry the tests read it through, and the "rgb" / "depth" exports of the
// HIP backend's ray caster.
#pragma once

#include "sim_c_api.h"
#include "cpu_render_bridge.hpp"

#include <madrona/render/ecs.hpp>
#ifndef SIM_BACKEND_REF_CPU
#include <madrona/mw_gpu.hpp>
#endif

#include <memory>

namespace simmgr {

// One per manager, made anew in makeConfig (sim_create runs makeConfig, then
// renderConfig on the HIP backend, then describeTensors).
struct RenderMgr {
    // ray caster output size as readRenderFlags saw it (0: no ray caster)
    uint32_t resolution = 0;
#ifdef SIM_BACKEND_REF_CPU
    std::unique_ptr<CpuRenderBridge> cpu;
#endif

    RenderMgr() = default;

    RenderMgr(const SimCreateArgs &args, uint32_t max_records_per_world,
              uint32_t views_per_world, uint32_t instances_per_world)
    {
#ifdef SIM_BACKEND_REF_CPU
        cpu = std::make_unique<CpuRenderBridge>(
            args.num_worlds, max_records_per_world, 64, views_per_world,
            instances_per_world);
#else
        (void)args; (void)max_records_per_world;
        (void)views_per_world; (void)instances_per_world;
#endif
    }

    // what Sim::Config takes
    const madrona::render::RenderECSBridge *bridge() const
    {
#ifdef SIM_BACKEND_REF_CPU
        return &cpu->bridge;
#else
        return nullptr;
#endif
    }

    // the renderer zeroes the append counters before every step
    void beginStep()
    {
#ifdef SIM_BACKEND_REF_CPU
        cpu->beginStep();
#endif
    }

    // CpuRenderBridge::records; -1 on the HIP backend or without a bridge
    int64_t records(int32_t kind, void *dst, uint64_t *keys_dst,
                    uint64_t max_records)
    {
#ifdef SIM_BACKEND_REF_CPU
        if (cpu == nullptr) return -1;
        return cpu->records(kind, dst, keys_dst, max_records);
#else
        (void)kind; (void)dst; (void)keys_dst; (void)max_records;
        return -1;
#endif
    }

#ifndef SIM_BACKEND_REF_CPU
    // The depth-only bit and the 8-bit resolution field of a simulator's
    // creation flags (every simulator has its own layout) into cfg; a field of
    // 0 means default_resolution.
    void readRenderFlags(madrona::CudaBatchRenderConfig &cfg, uint32_t flags,
                         uint32_t depth_only_bit, uint32_t resolution_shift,
                         uint32_t default_resolution)
    {
        using RenderMode = madrona::CudaBatchRenderConfig::RenderMode;
        cfg.renderMode = ((flags >> depth_only_bit) & 1u) != 0u ?
            RenderMode::Depth : RenderMode::RGBD;
        cfg.renderResolution = (flags >> resolution_shift) & 0xFFu;
        if (cfg.renderResolution == 0) cfg.renderResolution = default_resolution;
        resolution = cfg.renderResolution;
    }
#endif

    // The ray caster's outputs, if it is on: one image per view (rows of the
    // render-target table = output slots = rows of the camera table).
    template <typename List>
    void describeTensors(List &out, int64_t views, uint32_t rgb_slot,
                         uint32_t depth_slot) const
    {
        const int64_t R = resolution;
        if (R == 0) return;
        out.push_back({ "rgb", SIM_U8, { views, R, R, 4 }, rgb_slot });
        out.push_back({ "depth", SIM_F32, { views, R, R }, depth_slot });
    }
};

}

// CPU mode: the records of the last step as the reference appended them to the
// bridge (arrival order) + the (world << 32 | entity id) key of each.
// kind 0 = instances (64 B each), 1 = views (48 B each).  Returns the count (-1
// on HIP or with no bridge, -2 when max_records is too small).  A manager with
// a bridge states this once, after its SimTraits.
#define SIM_RENDER_BRIDGE_RECORDS(render_mgr)                                  \
    extern "C" SIM_API int64_t render_prep_bridge_records(                     \
        int32_t kind, void *dst, uint64_t *keys_dst, uint64_t max_records)     \
    {                                                                          \
        return (render_mgr).records(kind, dst, keys_dst, max_records);         \
    }
