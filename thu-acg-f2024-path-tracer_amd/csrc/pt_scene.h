// Host scene graph (the builder side of World / Hittable / BxDFMaterial / Texture): plain host data, no HIP type. pt_graph.cpp edits it,
// pt_flatten.cpp turns it into the tables of pt_types.h, pt_scene_upload.cpp puts those on the device; what lives there hangs off
// pt_scene::gpu (pt_scene_gpu.h).
#pragma once
#include <functional>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "pt_host_math.h"
#include "pt_types.h"

struct pt_camera;   // include/pt_amd.h

struct pt_ctx;      // pt_scene_gpu.h

namespace pt {
struct SceneGpu;    // pt_scene_gpu.h

int set_error(const std::string& msg);   // returns -1
const char* last_error();
// Experiment switches (PT_POOL_SLOTS, PT_SHADE_VARIANT, ...) are read only when PT_EXPERIMENT=1 is set: a release
// library's behaviour does not depend on stray environment variables, and an explicit option always wins over them.
const char* exp_env(const char* name);

enum ObjKind { OBJ_SPHERE, OBJ_QUAD, OBJ_CUBOID, OBJ_MESH, OBJ_INSTANCE };

struct HostTex {
    TexD d{};
    std::vector<uint8_t> image;   // TEX_IMAGE payload (RGB8)
    std::vector<float> image_f;   // TEX_IMAGE_F32 payload (RGB f32)
    bool is_rgb = false;
};
struct HostObj {
    ObjKind kind;
    int mat = -1;
    SphereD sphere{};
    std::vector<QuadD> quads;       // 1 (quad) or 6 (cuboid)
    std::vector<TriD> tris;         // mesh
    std::vector<TriAttr> tri_attr;  // mesh with normals and/or uvs
    bool has_normals = false, has_uvs = false;
    int child = -1;                 // instance
    InstD xf{};                     // (pt_instance_moving: the pose at time 0)
    InstMotionD motion{};           // the keys of pt_instance_moving; moves = 0 for pt_instance
    // An object may be placed in the world directly any number of times and wrapped by any number of instances, and an instance
    // may wrap an instance (Instance::new / World::add_object take an Arc<dyn Hittable>, instance.rs:20-30, world.rs:18-24).
};

struct HostGrid {                   // one grid-density medium (pt_mat_medium_grid): its descriptor (ofs filled at upload) and its samples
    GridD d{};
    std::vector<float> vals;
};

}  // namespace pt

struct pt_scene {
    pt_ctx* ctx = nullptr;
    pt::SceneGpu* gpu = nullptr;   // the device side (pt_scene_create / pt_scene_destroy); null in a scene that is only flattened on the host
    std::vector<pt::HostTex> tex;
    std::vector<pt::MatD> mats;
    std::vector<pt::HostObj> objs;
    std::vector<int> world_objects, world_lights;
    std::map<std::string, int> images;   // registered image name -> texture handle
    bool built = false;
    bool float_hdr = false;        // scene scripts / host mirrors load Radiance files as f32 textures (pt_scene_set_float_hdr)
    uint32_t n_prims = 0;
    uint32_t n_mesh_entries = 0;   // world-level triangle meshes (picks the K2 variant)
    bool motionless = false;       // no sphere moves (p1 == p2 everywhere) and no instance was made by pt_instance_moving: a ray's time never reaches an arithmetic result
    // motion (pt_instance_moving, pt_scene_set_shutter). has_moving_instance (set by scene_build): some placed object's chain
    // holds an instance made by pt_instance_moving. entry_boxes: the world boxes of the last build, six doubles per entry (pt_world_entry_box).
    bool has_moving_instance = false;
    double shutter_open = 0.0, shutter_close = 1.0;
    std::vector<double> entry_boxes;
    // the short-path pass: one flag per entry of the last build — the entry is SHADEABLE: a world-level sphere or quad without
    // an instance chain that does not move, its material diffuse without a normal map — and the global primitive ids of the flagged entries
    std::vector<uint8_t> entry_shadeable;
    std::vector<uint32_t> shade_prims;
    //  entry_at: the place of entry i in SceneD::entry_box; shade_entry: the entry of shade_prims[j]; shade_self_ok[j]: a quad
    // whose numbers keep the bound under which a bounce that left it cannot hit it again (k_short then does not test it)
    std::vector<uint32_t> entry_at, shade_entry;
    std::vector<uint8_t> shade_self_ok;
    bool motion_on() const {       // "in effect": the kernels' MOT forms run
        return has_moving_instance || ((shutter_open != 0.0 || shutter_close != 1.0) && !motionless);
    }
    uint32_t stack_need = 0;       // worst-case traversal stack entries of this scene's BVHs
    uint32_t device_bvh_min_tris = 1u << 19;   // meshes with at least this many triangles get their BVH built on the GPU (0 = never)
    uint32_t n_device_blas = 0, device_blas_depth = 0;   // meshes of the last build that the GPU builder handled, deepest of them
    uint32_t stack_need_extend2 = 0;   // ... for k_extend2, whose top-level walk is stackless when the entry list is walked flat
    // environment importance sampling (pt_scene_set_env_sampling): the mixture weight, and the f64 tables of ONE
    // environment texture (SceneGpu::env_tab), built at the first render or probe that needs them (pt_render.cpp env_tables) and kept until destroy
    double env_f = 0.0;
    int env_tab_tex = -1;          // texture the tables belong to (-1: none built)
    uint32_t env_tab_w = 0, env_tab_h = 0;
    double env_tab_z = 0.0;
    // participating media (pt_mat_medium). camera_medium: the medium material camera rays start in, -1 = none.
    // world_has_medium (set by scene_build): some world object's material is a medium.
    int camera_medium = -1;
    bool world_has_medium = false;
    // interior media and chromatic absorption (pt_mat_glass_set_interior, pt_mat_medium_tinted): MatD::p[0] of a glass = its
    // interior's handle + 1, p[7..9] of a medium = its absorption, p[10] = 1 for a tinted one. world_has_interior (set by scene_build): some
    // world object's material is a glass with an interior or a tinted medium.
    bool world_has_interior = false;
    bool interior_on() const {   // "in effect": the kernels' INT forms run (and with them MED and HET)
        return world_has_interior || (camera_medium >= 0 && mats[camera_medium].p[10] != 0.0);
    }
    bool media_on() const { return world_has_medium || camera_medium >= 0 || world_has_interior; }   // "in effect": the kernels' MED forms run
    // grid-density media (pt_mat_medium_grid): MatD::p[6] of a medium = its index here + 1. world_has_grid_medium (set by
    // scene_build): some world object's material is one.
    std::vector<pt::HostGrid> grids;
    bool world_has_grid_medium = false;
    bool grid_media_on() const {   // "in effect": the kernels' HET forms run
        return world_has_grid_medium || (camera_medium >= 0 && mats[camera_medium].p[6] != 0.0);
    }
    // exact light sampling (pt_scene_set_light_sampling): the kind, and what scene_build found in the lights list — a mesh or
    // sphere entry (kind 1 is then in effect), a light mesh whose area is 0 or not finite, the deepest light mesh tree
    int light_sampling = 0;        // 0 the reference's lights.sample / lights.pdf, 1 exact (the kernels' LSE forms)
    bool lights_have_mesh_or_sphere = false, light_mesh_bad_area = false;
    uint32_t light_blas_depth = 0;
    bool light_sampling_on() const { return light_sampling == 1 && lights_have_mesh_or_sphere; }   // "in effect"
    // spectral dispersion (pt_mat_glass_set_dispersion): MatD::p[1..3] of a glass = the Cauchy b, inv2(0.58756) and its Abbe
    // number (0 = off). world_has_dispersion (set by scene_build): some world object's material is a glass with an Abbe number > 0.
    // (the weight table W[DSP_BINS][3] on the device: SceneGpu::disp_w)
    bool world_has_dispersion = false;
    bool dispersion_on() const { return world_has_dispersion; }   // "in effect": the kernels' DSP forms run
    // punctual lights (pt_light_point / pt_light_spot / pt_light_directional): the list as the calls formed it, the selector's
    // share of the punctual branch, and the number of lights of the last build (the device list: SceneD::punctual)
    std::vector<pt::PunctualD> punctual;
    double punctual_f = 0.5;
    uint32_t n_punctual_built = 0;
    bool punctual_on() const { return n_punctual_built != 0u; }   // "in effect": the kernels' PLT forms run
    // light shafts (pt_scene_set_punctual_media): the option that lets punctual lights and participating media be in effect together
    int punctual_media = 0;
    // the light grid (pt_scene_set_punctual_selection / pt_scene_set_punctual_grid): the settings wait for the next build like
    // the list; grid_built: what the last build used (cells = 0: the grid is not in effect; the table: SceneD::punctual_cdf)
    int punctual_selection = 0;    // 0 uniform, 1 the light grid
    uint32_t grid_dims_set[3] = {0u, 0u, 0u};   // all 0: automatic
    bool grid_box_given = false;
    double grid_box_set[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    pt::PunctualGridBuild grid_built{};
    double grid_build_ms = 0.0;    // the table kernel's time at the last build (PT_VERBOSE prints it)
    int projection = 0;            // pt_scene_set_projection: 0 perspective, 1 orthographic, 2 fisheye, 3 panorama (CamD::projection)
    int sampler = 0;               // pt_scene_set_sampler: 0 independent (Philox), 1 Owen-scrambled Sobol (the kernels' QMC forms)
};

namespace pt {
int scene_build(pt_scene* s);   // flatten + BVH + upload (pt_scene_upload.cpp)
// pt_graph.cpp: the record constructors the entry points share with the flattener and the upload
void pose_of_keys(const InstMotionD& k, double time, InstD& xf);      // the pose of a moving instance's keys at `time`
host::Box xform_box(const host::Box& b, const InstD& m);              // box of the transformed box
host::Box swept_box(const host::Box& b, const InstMotionD& k);        // ... under a moving instance over every time in [0, 1]
bool grid_box_ok(const double b[6]);                                  // a light grid's box: finite, hi >= lo
PunctualGridD grid_descriptor(const double box[6], const uint32_t dims[3], uint32_t n);
void dispersion_weights(double w[DSP_BINS][3]);   // the weight table of pt_mat_glass_set_dispersion's rule (host, f64)
double dispersion_ior(const MatD& glass, double lambda_nm);   // n(lambda) of a dispersive glass as the device computes it
// pt_render.cpp, shared with the probes (pt_probe.cpp): the device camera of a render
int make_camd(pt_scene* s, const pt_camera* cam, CamD& dc);
// pt_probe.cpp: the one path of the probes and the u8 resolves. Host inputs go to the device, `launch` enqueues its kernel on the
// context's stream given the device pointers (inputs in the order listed), the launch error is checked, `out_bytes` come back and the
// stream is synchronised. 0, or -1 with the error set. An empty output (n == 0) is no device work at all.
struct ProbeIn {
    const void* host;
    size_t bytes;
};
int run_probe(pt_ctx* ctx, std::initializer_list<ProbeIn> in, void* out, size_t out_bytes, const std::function<void(void* const* d_in, void* d_out)>& launch);
}
