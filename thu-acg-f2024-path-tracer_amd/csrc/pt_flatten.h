// The flattener (host-only): a scene graph (pt_scene.h) into the host arrays of the device tables (pt_types.h) — placements, one BVH per
// mesh object, the top level, the flat walk's records, textures folded into materials. Pure f64 host code over std::vector: it reads the
// graph and the settings of `s`, writes the derived host fields of `s` (world_has_*, entry_*, shade_*, stack_need, ...) and never
// touches s.gpu. pt_scene_upload.cpp puts the result on the device; tools/scene_host_check.cpp runs it on a CPU.
#pragma once
#include <functional>
#include <vector>

#include "pt_scene.h"

namespace pt {

struct DeviceBlas {                 // what a device builder hands back for one mesh (pt_bvh_device.hip)
    std::vector<BvhNode> nodes;     // node 0 = root; child references are LOCAL: REF_NODE | index into `nodes`,
                                    // REF_TRIS | (count-1) << 27 | first position in `order`
    std::vector<uint32_t> order;    // BLAS (leaf) order: position -> face index of the mesh
    int depth = 0;                  // deepest leaf, counted like the host builder's depth_reached
};
// build_blas_device's arguments without the stream (pt_bvh_device.h). Null, or a call that returns false: the host builder takes the mesh.
using BlasHook = std::function<bool(const TriD* tris, uint32_t n, const double mesh_lo[3], const double mesh_hi[3], uint32_t leaf_max, uint32_t max_depth,
                                    uint32_t median_below, DeviceBlas& out)>;

struct FlatScene {                  // one array per SceneD pointer, in upload order, then the scalars of the view
    std::vector<BvhNode> nodes;
    std::vector<Entry> entries;
    std::vector<PrimRef> prims;
    std::vector<SphereD> spheres;
    std::vector<QuadD> quads;
    std::vector<TriD> tris;
    std::vector<uint32_t> tri_gid;
    std::vector<InstD> insts;
    std::vector<TexD> tex;
    std::vector<MatD> mats;
    std::vector<uint8_t> atlas;
    std::vector<float> atlas_f;
    std::vector<uint32_t> lights;
    std::vector<EntryBox> entry_box;
    std::vector<CuboidBox> cuboid_box;
    std::vector<double> light_cdf;          // the light meshes' running area sums, one table per mesh object
    std::vector<TriAttr> tri_attr;          // parallel to tris; uploaded when any_attr
    std::vector<InstMotionD> inst_motion;   // parallel to insts; uploaded when any_moving
    std::vector<GridD> grids;               // the grid-density media's table and their samples, one array
    std::vector<float> grid_vals;
    uint32_t tlas_root = REF_EMPTY;
    float tlas_extent = 0.0f;
    uint32_t tlas_flat = 0, flat_pairs = 0;
    PunctualGridBuild grid{};               // the light grid's box and dims (cells = 0: not in effect); its table is formed on the device
    bool any_attr = false, any_moving = false;
    int max_blas_depth = 0, tlas_depth = 0;
};

// 0, or -1 with the error set. A refused build leaves in `s` what the steps before the refusal wrote.
int flatten(pt_scene& s, const BlasHook& device_blas, FlatScene& out);
// The fields only a finished build sets (n_prims, n_mesh_entries, n_punctual_built, has_moving_instance, motionless, stack_need_extend2,
// grid_built, built): the last step of a build, after whatever its caller does with `f` (the upload) has succeeded.
void finish_build(pt_scene& s, const FlatScene& f);
// FNV-1a over the arrays and scalars of `f` in the order above, field by field (no padding enters). Two builds flattened alike print the
// same number under PT_VERBOSE.
uint64_t flat_checksum(const FlatScene& f);

}  // namespace pt
