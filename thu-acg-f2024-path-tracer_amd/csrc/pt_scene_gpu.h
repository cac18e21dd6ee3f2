// The GPU side of a scene and of a context: everything of the host runtime that holds device memory or names a HIP type. pt_scene (pt_scene.h)
// is plain host data and points here (pt_scene::gpu: made by pt_scene_create, freed by pt_scene_destroy); every member below owns its
// memory (pt_devmem.h), so the struct's destructor is the implicit one.
#pragma once
#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "pt_devmem.h"
#include "pt_scene.h"

struct pt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int n_cus = 0;
    std::string name;
};

namespace pt {

struct DeviceBuffers {          // the arrays of the last build (pt_scene_upload.cpp) and the kernels' view of them
    std::vector<DevMem> allocs;
    SceneD view{};
    void release();
};

struct SceneGpu {
    DeviceBuffers dev;
    // buffers cached across calls (pt_devmem.h GrowBuf: grown on demand, freed with the scene). A call sizes what it carves out of one
    // from its own needs, never from the cached capacity.
    GrowBuf pool_mem;          // the path pool of a render (pt_render.cpp bind_pool)
    GrowBuf tile_accum;        // dynamic mode: the frame accumulator in tile order (PoolD::accum_tiled)
    GrowBuf compact_scratch;   // the end-of-frame compaction's hole / mover lists + counters (pt_render.cpp)
    GrowBuf pixel_list;        // pt_render_pixels: the device pixel list (tiled order)
    GrowBuf sky_mem;           // the sky pass: counts, boxes, tile flags, the sure-sky tile list (pt_render.cpp classify_sky; the tile map is in tile_accum)
    GrowBuf short_mem;         // the short-path pass's hard list (pt_render.cpp run_short; its tile list and the shadeable ids are in sky_mem)
    GrowBuf env_tab;           // environment importance sampling: H * (W + 1) row prefix sums, then H + 1 row-total prefix sums (EnvTabD), doubles; pt_scene::env_tab_* say whose
    DevMem disp_w;             // spectral dispersion: the weight table W[DSP_BINS][3], uploaded at the first render or probe that needs it (dispersion_table)
    DevMem d_counters;         // a render's CountersD, and its pinned host copy (pt_render.cpp bind_pool allocates both)
    GrowBuf h_counters{true};
    CountersD* counters() const { return d_counters.as<CountersD>(); }
    CountersD* host_counters() const { return h_counters.as<CountersD>(); }
};

double* dispersion_table(pt_scene* s, hipStream_t st);   // SceneGpu::disp_w, uploaded if need be; null (error set) when that fails
// pt_render.cpp, shared with the probes (pt_probe.cpp): the environment-sampling tables of a render's map
int env_tables(pt_scene* s, const CamD& dc, hipStream_t st, EnvTabD& e);

}  // namespace pt
