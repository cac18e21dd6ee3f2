// The device side of a scene build: the flattened scene (pt_flatten.h) into device memory, the light grid's table, the kernels' view.
// See pt_scene_gpu.h.
#include "pt_scene_gpu.h"
#include "pt_bvh_device.h"
#include "pt_flatten.h"
#include "pt_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "../../include/pt_amd.h"

using namespace pt;

namespace pt {
bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}
void DeviceBuffers::release() {
    allocs.clear();   // (each frees itself: pt_devmem.h DevMem)
    view = SceneD{};
}
double* dispersion_table(pt_scene* s, hipStream_t st) {
    DevMem& d = s->gpu->disp_w;
    if (d) return d.as<double>();
    double w[DSP_BINS][3];
    dispersion_weights(w);
    if (!d.alloc(sizeof w, "hipMalloc(dispersion weights)")) return nullptr;
    if (!hip_ok(hipMemcpyAsync(d.as<double>(), w, sizeof w, hipMemcpyHostToDevice, st), "hipMemcpy(dispersion weights)") ||
        !hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize(dispersion weights)")) {   // (`w` is on this stack)
        d.release();
        return nullptr;
    }
    return d.as<double>();
}
}  // namespace pt

// (among the scene-graph setters of pt_graph.cpp, the one that also edits the device view)
extern "C" int pt_scene_set_punctual_fraction(pt_scene* s, double f) {
    if (!s) return set_error("pt_scene_set_punctual_fraction: null scene");
    if (!std::isfinite(f) || !(0.0 < f && f < 1.0)) return set_error("pt_scene_set_punctual_fraction: the fraction must be finite with 0 < f < 1");
    s->punctual_f = f;
    s->gpu->dev.view.punctual_f = f;   // (read by the PLT forms only: a scene without punctual lights renders the same bits whatever f is)
    return 0;
}
extern "C" int pt_world_build(pt_scene* s) { return scene_build(s); }

namespace {
template <class T>
bool upload(DeviceBuffers& dev, const std::vector<T>& v, const T*& out) {
    out = nullptr;
    DevMem m;
    if (!m.alloc(std::max<size_t>(v.size(), 1) * sizeof(T), "hipMalloc(scene)")) return false;
    void* p = m.as<void>();
    dev.allocs.push_back(std::move(m));
    if (!v.empty() && !hip_ok(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy(scene)")) return false;
    out = (const T*)p;
    return true;
}
// The light grid's table: one row of n doubles per cell, formed on the GPU from the list just uploaded; PT_VERBOSE times the kernel
bool build_light_grid(pt_scene* s, const PunctualGridBuild& gb, SceneD& v) {
    const uint32_t n = (uint32_t)s->punctual.size();
    DevMem table;
    if (!table.alloc((size_t)gb.cells * n * sizeof(double), "hipMalloc(light grid)")) return false;
    double* t = table.as<double>();
    s->gpu->dev.allocs.push_back(std::move(table));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool timed = exp_env("PT_VERBOSE") && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    if (timed) (void)hipEventRecord(e0, s->ctx->stream);
    launch_punctual_grid(v.punctual, n, gb, t, !exp_env("PT_GRID_DIRECT"), s->ctx->stream);
    if (timed) (void)hipEventRecord(e1, s->ctx->stream);
    const bool ok = hip_ok(hipGetLastError(), "kernel launch") && hip_ok(hipStreamSynchronize(s->ctx->stream), "hipStreamSynchronize");
    float ms = 0.0f;
    if (ok && timed && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) {
        s->grid_build_ms = ms;
        fprintf(stderr, "[pt] light grid: %u x %u x %u cells x %u lights, %zu bytes, built in %.3f ms (%s)\n", gb.dims[0], gb.dims[1], gb.dims[2], n,
                (size_t)gb.cells * n * sizeof(double), ms, exp_env("PT_GRID_DIRECT") ? "direct stores" : "staged through LDS");
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    v.punctual_cdf = t;
    v.punctual_grid = grid_descriptor(gb.box, gb.dims, n);
    return ok;
}
}  // namespace

int pt::scene_build(pt_scene* s) {
    if (!s->ctx) return set_error("scene has no context");
    if (!hip_ok(hipSetDevice(s->ctx->device), "hipSetDevice")) return -1;
    DeviceBuffers& dev = s->gpu->dev;
    dev.release();
    s->built = false;

    FlatScene f;
    const hipStream_t st = s->ctx->stream;
    const BlasHook device_blas = [st](const TriD* tris, uint32_t n, const double lo[3], const double hi[3], uint32_t leaf_max, uint32_t max_depth, uint32_t median_below,
                                      DeviceBlas& out) { return build_blas_device(tris, n, lo, hi, leaf_max, max_depth, median_below, out, st); };
    if (flatten(*s, device_blas, f) != 0) return -1;
    if (exp_env("PT_VERBOSE")) {
        fprintf(stderr, "[pt] BVH: top-level depth %d, deepest mesh tree %d, %zu nodes, %zu triangles\n", f.tlas_depth, f.max_blas_depth, f.nodes.size(), f.tris.size());
        fprintf(stderr, "[pt] flat scene checksum %016llx\n", (unsigned long long)flat_checksum(f));
    }

    SceneD v{};
    bool ok = upload(dev, f.nodes, v.nodes) && upload(dev, f.entries, v.entries) && upload(dev, f.prims, v.prims) &&
              upload(dev, f.spheres, v.spheres) && upload(dev, f.quads, v.quads) && upload(dev, f.tris, v.tris) &&
              upload(dev, f.tri_gid, v.tri_gid) && upload(dev, f.insts, v.insts) && upload(dev, f.tex, v.tex) &&
              upload(dev, f.mats, v.mats) && upload(dev, f.atlas, v.atlas) && upload(dev, f.atlas_f, v.atlas_f) && upload(dev, f.lights, v.lights) &&
              upload(dev, f.entry_box, v.entry_box) && upload(dev, f.cuboid_box, v.cuboid_box) && upload(dev, f.light_cdf, v.light_cdf);
    if (ok && f.any_attr) ok = upload(dev, f.tri_attr, v.tri_attr);
    if (ok && f.any_moving) ok = upload(dev, f.inst_motion, v.inst_motion);
    if (ok && !f.grids.empty()) ok = upload(dev, f.grids, v.grids) && upload(dev, f.grid_vals, v.grid_vals);
    if (ok && !s->punctual.empty()) ok = upload(dev, s->punctual, v.punctual);
    if (ok && f.grid.cells != 0u) ok = build_light_grid(s, f.grid, v);
    if (!ok) {
        dev.release();
        return -1;
    }
    v.tlas_root = f.tlas_root;
    v.tlas_extent = f.tlas_extent;
    v.n_entries = (uint32_t)f.entries.size();
    v.n_prims = (uint32_t)f.prims.size();
    v.n_lights = (uint32_t)f.lights.size();
    v.n_punctual = (uint32_t)s->punctual.size();
    v.punctual_f = s->punctual_f;
    v.tlas_flat = f.tlas_flat;
    v.flat_pairs = f.flat_pairs;
    dev.view = v;
    finish_build(*s, f);
    return 0;
}
