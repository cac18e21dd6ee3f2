// Flattened scene + path-pool layout shared by the host scene builder and the HIP kernels.
// Everything the kernels read lives in HBM as plain arrays of these PODs (records for the per-path
// state and for the small read-only scene tables that sit in L2).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pt {

// ---- BVH -----------------------------------------------------------------------------
// One node format for the top-level tree (over world objects) and every per-mesh tree.
// Boxes are stored as f32 rounded OUTWARD from the padded f64 bounds (conservative); the slab
// test runs in f32 with a per-ray error margin (pt_k_trace.h, slab_f32) — box tests only have
// to be conservative, the f64 primitive tests decide the result. 64 B = four 16-B loads per visit.
// Child reference (32 bit):
//   00xx.. internal node index
//   01cc cfff.. triangle leaf: ccc = count-1 (1..8), f = first triangle (BLAS order)
//   10xx.. world entry index (top-level leaf, always exactly one entry)
//   0xFFFFFFFF empty slot, 0xC0000000 "leave instance" sentinel (stack only)
struct alignas(16) BvhNode {
    float lo0[3], hi0[3];
    float lo1[3], hi1[3];
    uint32_t child0, child1;
    uint32_t pad0, pad1;
};
constexpr uint32_t REF_TYPE_MASK = 0xC0000000u;
constexpr uint32_t REF_NODE = 0x00000000u;
constexpr uint32_t REF_TRIS = 0x40000000u;
constexpr uint32_t REF_ENTRY = 0x80000000u;
constexpr uint32_t REF_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t REF_LEAVE_INSTANCE = 0xC0000000u;
constexpr int TRAVERSAL_STACK = 32;     // LDS entries per lane
constexpr int MAX_BLAS_DEPTH = 20;      // enforced by the host builder
constexpr int MAX_TLAS_DEPTH = 10;

// ---- geometry ------------------------------------------------------------------------
enum PrimKind : uint32_t { PRIM_SPHERE = 0, PRIM_QUAD = 1, PRIM_TRI = 2 };
enum EntryKind : uint32_t { ENTRY_SPHERE = 0, ENTRY_QUAD = 1, ENTRY_CUBOID = 2, ENTRY_MESH = 3 };
constexpr uint32_t PRIM_HAS_NORMALS = 1u << 8, PRIM_HAS_UVS = 1u << 9;
// A SPHERE whose material can read HitD::u / v. The scene build sets it when the material has a normal map (nmap_tex >= 0), when its
// colour texture tree — through checker children — holds an image texture (TEX_IMAGE, TEX_IMAGE_F32), or when it is a mix with such a
// child at either nesting level. Nothing else in k_shade reads a hit's (u, v) (fetch_tex's colour lookup and finish_hit's normal
// map are the two places), so k_shade computes a sphere's (u, v) — dev_acos, dev_atan2, two divisions — only where the bit is set and
// passes zeros elsewhere: the host proves the value unused, as it does for the Philox blocks nobody reads (CamD::motionless).
// Quads and triangles have their (u, v) from the intersection itself; the bit is not set for them.
constexpr uint32_t PRIM_NEEDS_UV = 1u << 10;
constexpr uint32_t PRIM_MAT_KIND_SHIFT = 16;   // PrimRef::kind bits 16..23: MatKind of the primitive's material (k_shade's class sort)

struct PrimRef {         // indexed by GLOBAL primitive id (lights list first, then objects)
    uint32_t kind;       // PrimKind | PRIM_HAS_*
    uint32_t index;      // index into spheres[] / quads[] / tris[]
    uint32_t mat;
    int32_t inst;        // OUTERMOST instance of the placement's chain, or -1
};
struct Entry {           // one per world-level object (lights list first, then objects)
    uint32_t kind;       // EntryKind
    uint32_t first_prim; // global id of its first primitive
    int32_t inst;        // OUTERMOST instance of the placement's chain, or -1
    uint32_t blas_root;  // node index (ENTRY_MESH); several placements of one mesh share the tree and its triangles
    float extent;        // ENTRY_MESH: max |coordinate| of the mesh's (local-space) BVH boxes
    uint32_t n_prims;    // 1 (sphere, quad), 6 (cuboid) or the triangle count (mesh)
    uint32_t pad[2];     // pad[0]: a MESH entry of the lights list: first element of its area table in SceneD::light_cdf
};
// Flat top-level walk (SceneD::tlas_flat): everything a step of the walk needs in ONE 64-byte record, i.e. one scalar load — the
// entry's world-space box (padded and rounded outward like the node boxes), a copy of its Entry, and for spheres / quads /
// cuboids the record index of the (first) primitive, so that neither Entry nor PrimRef has to be fetched first: with a
// handful of waves per SIMD every dependent scalar load is ~200 exposed cycles, and the walk made three per entry.
struct EntryBox {
    float lo[3], hi[3];
    uint32_t entry;      // index into SceneD::entries
    uint32_t kind;       // EntryKind                                    -- Entry's fields from here
    uint32_t first_prim;
    int32_t inst;
    uint32_t blas_root;
    float extent;
    uint32_t n_prims;
    uint32_t prim_kind;  // PRIM_SPHERE / PRIM_QUAD of the entry's primitives, or ENTRYBOX_VIA_PRIMREF: look them up in prims[]
    uint32_t prim_index; // spheres[] / quads[] index of primitive first_prim (the faces of a cuboid follow consecutively)
    uint32_t pad;
};
constexpr uint32_t ENTRYBOX_VIA_PRIMREF = 0xFFFFFFFFu;
// Parallel to SceneD::entry_box, meaningful for ENTRY_CUBOID records: the cuboid's OBJECT-space box (cuboid.rs:11-58 builds its six
// quads on the faces of [min, max]), f32 rounded outward like every stored box; EntryBox::extent then holds max |coordinate| of
// it. The flat walk slab-tests the object-space ray against it and only runs the exact quad tests of the faces the ray can
// enter or leave through (flat_top_level, "face culling"): typically two of the six.
struct CuboidBox {
    float lo[3], hi[3];
    float pad[2];
};
struct SphereD { double r, p1[3], p2[3]; };
struct QuadD { double q[3], u[3], v[3], w[3], n[3], d; };
struct TriD { double v0[3], v1[3], v2[3]; };
struct TriAttr { double n[3][3]; double uv[3][2]; };   // only when the mesh has them
// One Instance of a placement (instance.rs:12-30): forward transform (columns c0..c2, translation t) and its analytic rigid
// inverse. Instances nest (Instance::new takes any Hittable): a placement is a CHAIN of them — `inner` is the next one
// towards the object, `outer` the next one towards the world, -1 at the ends. Every placement owns its chain.
struct InstD {
    double c0[3], c1[3], c2[3], t[3], i0[3], i1[3], i2[3], it[3];
    int32_t inner, outer;
};
// The two keys of an instance made by pt_instance_moving (the rule: pt_amd.h), parallel to SceneD::insts; the differences
// are formed once on the host. InstD holds the pose at time 0; the pose at a ray's time is rebuilt per lane by inst_at (pt_dev_geom.h)
// with pt_instance's operation sequence. moves = 0: a pt_instance record, left as stored. spins = 0 (angle0 == angle1): the stored
// rotation columns stay, only t and it are recomputed.
struct InstMotionD {
    double axis[3], angle0, dangle, tr0[3], dtr[3];
    uint32_t moves, spins;
};

// ---- textures / materials ------------------------------------------------------------
// TEX_IMAGE_F32: ImageTexture WITHOUT the `.to_rgb8()` squash of texture.rs:67 — the decoder's f32 samples (a Radiance .hdr decodes to
// Rgb32F) live in SceneD::atlas_f and the lookup of texture.rs:73-91 returns them widened to f64 (behind a flag).
enum TexKind : uint32_t { TEX_SOLID_RGB = 0, TEX_SOLID_F = 1, TEX_CHECKER = 2, TEX_IMAGE = 3, TEX_IMAGE_F32 = 4 };
struct TexD {
    uint32_t kind, t1, t2, w, h;
    uint32_t flat;       // TEX_CHECKER whose two children are solid: their values sit in c1 / c2 — one level less in the chain of
                         // DEPENDENT loads primitive -> material -> texture -> child texture (~700 cycles each in k_shade).
                         // (Also copying the descriptors into the material record made k_shade spill 384 B per lane.)
    uint64_t ofs;        // byte offset into the RGB8 atlas (TEX_IMAGE) / element offset into the f32 atlas (TEX_IMAGE_F32)
    double v[3];
    double inv_scale;
    double c1[3], c2[3];
};
enum MatKind : uint32_t { MAT_DIFFUSE = 0, MAT_METAL = 1, MAT_GLASS = 2, MAT_PRINCIPLED = 3, MAT_LIGHT = 4,
                          MAT_SHEEN = 5, MAT_CLEARCOAT = 6, MAT_MIX = 7, MAT_KINDS = 8,
                          // A homogeneous participating medium (pt_mat_medium): p[0] = density (sigma_t), p[1] = the
                          // Henyey-Greenstein g, p[2..4] = the single-scattering albedo, p[5] = 1 when a world object carries it (scene_build). Not one of the MAT_KINDS sort classes: the
                          // primitives of a medium's boundary carry MAT_GLASS in PrimRef::kind (MEDIUM_SORT_KIND), so K2's result word
                          // and the default k_shade forms' sort stay what they were; only k_shade's MED forms look at MatD::kind.
                          // A grid-density medium (pt_mat_medium_grid) is the same kind with p[6] = its row of SceneD::grids + 1
                          // (0 = homogeneous) and p[0] = its majorant mu; only k_shade's HET forms and the probe read p[6].
                          // A tinted medium (pt_mat_medium_tinted) keeps its absorption coefficients in p[7..9] (zero for every
                          // other medium) and p[10] = 1; a MAT_GLASS keeps its interior medium's index + 1 in p[0] (pt_mat_glass_set_interior,
                          // 0 = none). Only k_shade's INT forms and the probe read these.
                          MAT_MEDIUM = 9 };
constexpr uint32_t MEDIUM_SORT_KIND = MAT_GLASS;
// The medium a path is in travels in the upper bits of its record's bounce word (RayRec's in the compact layout, else PathRec's):
// word = bounce | (material index + 1) << MEDIUM_SHIFT, 0 = no medium. Only the MED forms of k_init / k_shade pack and unpack it;
// without media in effect the field is zero and the word is the bounce number, as before. The host refuses a medium material whose
// index does not fit and a max_depth that reaches into the field (pt_mat_medium, pt_render).
constexpr uint32_t MEDIUM_SHIFT = 20, MEDIUM_BOUNCE_MASK = (1u << MEDIUM_SHIFT) - 1u, MEDIUM_MAX_MATS = 4094;
// Spectral dispersion (pt_mat_glass_set_dispersion): a dispersive MAT_GLASS keeps the Cauchy coefficient b in p[1], inv2(0.58756)
// in p[2] and its Abbe number in p[3] (0 = not dispersive; glass uses none of them otherwise, and p[0] is the interior). A path's MONO flag —
// it has been weighted by its wavelength's row of the weight table — is bit 31 of its bounce word, which the non-MED forms leave free. Only
// the DSP forms of k_shade pack and unpack it; a camera ray's word is 0, so K1 has no DSP form. The host refuses a max_depth that reaches
// the bit (pt_render). The weight table W[DSP_BINS][3] (f64, the same for every scene) reaches the DSP forms through the `col` pointer of
// their EnvTabD argument, which only the ENV forms read otherwise.
constexpr uint32_t DSP_MONO_BIT = 1u << 31, DSP_BOUNCE_MASK = DSP_MONO_BIT - 1u;
constexpr int DSP_BINS = 64;
// Punctual lights (pt_light_point / pt_light_spot / pt_light_directional; the rule: pt_amd.h). One record per light, formed
// on the host: kind 0 point (I = power / 4 pi), 1 spot (axis = normalize(target - position), the two cosines from the host's deterministic
// cosine), 2 directional (axis = the way the light travels, I = the irradiance). A path on its SHADOW segment — the ray from a surface
// towards light k that the next visit of K3 resolves — carries the flag in bit 31 of its bounce word and k in bits 20..30, which the plain
// mode leaves free as it does DSP's MONO bit. Only the PLT forms of k_shade pack and unpack them; a camera ray's word is 0, so K1 has no PLT
// form. The host refuses a max_depth that reaches the field (pt_render).
struct PunctualD {
    uint32_t kind, pad;
    double pos[3], axis[3], I[3], cos_i, cos_o;
};
constexpr uint32_t PLT_MAX_LIGHTS = 2048, PLT_SHADOW_BIT = 1u << 31, PLT_INDEX_SHIFT = 20, PLT_INDEX_MASK = PLT_MAX_LIGHTS - 1u,
                   PLT_BOUNCE_MASK = (1u << PLT_INDEX_SHIFT) - 1u;
// The light grid (pt_scene_set_punctual_selection kind 1; the rule: pt_amd.h): a uniform world-space grid of n[0] x n[1] x n[2]
// cells over the box that starts at lo; inv = n / (hi - lo) per axis (0 on an axis of extent 0). Cell (ix, iy, iz) has index (iz * n[1] + iy)
// * n[0] + ix, and row `cell` of the table (SceneD::punctual_cdf) is the cell's CDF over the whole list: `stride` doubles, the list's length.
struct PunctualGridD {
    double lo[3], inv[3];
    uint32_t n[3], stride;
};
struct PunctualGridBuild {   // what the build kernel and pt_punctual_grid_row form a row from: the box (lo.xyz, hi.xyz), the dims, their product
    double box[6];
    uint32_t dims[3], cells;
};
constexpr uint64_t PLT_GRID_MAX_ENTRIES = 1ull << 25;   // cells x lights: 256 MiB of doubles
constexpr uint32_t PLT_GRID_MAX_DIM = 64, PLT_GRID_AUTO_RES = 16;
// Light shafts (pt_scene_set_punctual_media): punctual lights and participating media in effect together. Medium AND shadow
// segment travel in the one bounce word: the medium stays in bits 20..31 (MEDIUM_SHIFT — a camera ray's word is the MED forms', so K1 has no
// form of its own), the SHADOW flag is bit 19, the light index bits 8..18, the bounce number bits 0..7. Only the forms of k_shade that have
// both PLT and a media mode pack and unpack this layout; the host refuses a max_depth above SHF_BOUNCE_MASK (pt_render).
constexpr uint32_t SHF_SHADOW_BIT = 1u << 19, SHF_INDEX_SHIFT = 8, SHF_BOUNCE_MASK = (1u << SHF_INDEX_SHIFT) - 1u;
static_assert((PLT_INDEX_MASK << SHF_INDEX_SHIFT) < SHF_SHADOW_BIT && SHF_SHADOW_BIT < (1u << MEDIUM_SHIFT), "the fields of a light-shaft bounce word do not overlap");
// THE shading mode of a render: which of the mutually exclusive features is in effect (the rules: pt_amd.h; which one a scene gets, or why
// it gets none: pt_render.cpp render_mode). k_shade and shade_slot are compiled once per mode; "the X forms" are the kernels whose mode has X:
//   PLAIN  none of them
//   ENV    environment importance sampling; the kernel's EnvTabD argument holds its tables
//   MED    participating media (§12)
//   HET    MED, and grid-density media (§13): a homogeneous medium is rendered with MED's bits
//   INT    MED and HET, and interior media / chromatic absorption (§14)
//   LSE    exact light sampling (§15); needs a lights list
//   DSP    spectral dispersion (§16); the `col` pointer of the kernel's EnvTabD argument is the weight table
// Nothing else combines: MED < HET < INT nest, every other pair excludes each other. The pixel list, the Sobol sampler and the lights list
// are orthogonal to the mode (ShadeForm, pt_kernels.h).
enum ShadeMode { MODE_PLAIN, MODE_ENV, MODE_MED, MODE_HET, MODE_INT, MODE_LSE, MODE_DSP, N_SHADE_MODES /* their number, not a mode */ };
constexpr bool mode_has_media(ShadeMode m) { return m == MODE_MED || m == MODE_HET || m == MODE_INT; }
constexpr bool mode_has_grid(ShadeMode m) { return m == MODE_HET || m == MODE_INT; }
constexpr bool mode_has_table(ShadeMode m) { return m == MODE_ENV || m == MODE_DSP; }
// The forms of K1 / K3 the sky pass can run with (pt_render.cpp classify_sky switches the pass off for every other): the whole
// frame in the plain mode, independent sampler, nothing moving, a two-wave shape of k_shade (every shape but the three-wave experiments).
// Only these read the tile map (pt_k_common.h work_to_pixel); every other form's code is what it was before the pass existed.
// (`motion`: the form has a trailing bool — MOT, or PLT of the punctual lights — that keeps the pass off.)
constexpr bool sky_pass_form(bool list, ShadeMode m, bool qmc, bool motion, bool two_waves = true) { return !list && m == MODE_PLAIN && !qmc && !motion && two_waves; }
constexpr uint32_t CLASS_MISS = 0u, CLASS_IDLE = 1u + MAT_KINDS, CLASS_DEAD = 2u + MAT_KINDS, N_CLASSES = 3u + MAT_KINDS;
// MAT_SHEEN: p[0..2] = base colour, p[3] = sheen_tint (sheen.rs). MAT_CLEARCOAT: alpha_g (clearcoat.rs).
// MAT_MIX: p[0] = t, color_tex / rough_tex hold the two child MATERIAL indices (mix.rs; children are leaves).
struct MatD {
    uint32_t kind;
    int32_t color_tex, rough_tex, nmap_tex;
    double ior;
    // principled.rs:45-58 order: metallic, roughness, subsurface, specular, specular_tint,
    // ior, spec_trans, sheen, sheen_tint, clearcoat, clearcoat_gloss
    double p[11];
    double lobe_w[4], lobe_p[4], alpha_g;   // principled.rs:75-100, precomputed on the host
    // A SOLID colour / roughness texture's value, copied here by the scene build: the material record then answers without the
    // texture descriptor — one level less in k_shade's chain of dependent loads (primitive -> material -> texture). Filled for
    // MAT_DIFFUSE / METAL / GLASS / PRINCIPLED / LIGHT; a mix's children are looked up the long way.
    uint32_t color_solid, rough_solid;
    double color_v[3], rough_v;
};

// One grid-density medium (pt_mat_medium_grid; the rule is in include/pt_amd.h): sigma(x) = scale * V(x), V the trilinear
// blend of the f32 samples vals[ofs + (k*ny + j)*nx + i] at the cell centres of the world-space box [lo, hi]. cells[a] = n_a / (hi_a - lo_a);
// mu = scale * max(values), the majorant delta tracking runs at.
struct GridD {
    uint32_t nx, ny, nz, pad;
    uint64_t ofs;            // first value of this grid in SceneD::grid_vals
    double lo[3], hi[3], cells[3];
    double scale, mu;
};

// ---- camera --------------------------------------------------------------------------
struct CamD {
    double center[3], pixel00[3], pixel_du[3], pixel_dv[3], dof_right[3], dof_up[3];
    double blur_strength;
    double env_color[3];
    double two_pi_scale;     // rand's UniformFloat scale for gen_range(0.0..=2pi)
    uint32_t width, height, max_depth, env_is_map;
    int32_t env_tex;
    uint32_t n_lights;
    uint32_t lens_zero;      // defocus radius 0 (dof_right = dof_up = 0, no -0.0 in center): the lens point is `center` exactly
    uint32_t motionless;     // no moving sphere in the scene: Ray::time is drawn (camera.rs:165) but its value is never used
    uint32_t medium;         // the medium camera rays start in: material index + 1, 0 = none (pt_scene_set_camera_medium; read by the MED forms only)
    // the projection (pt_scene_set_projection; the rule is in include/pt_amd.h). Everything below is read by kinds 1-3 only:
    // kind 0 (PROJ_PERSPECTIVE) reads `projection` and then what it read before the setting existed (generate_ray, pt_dev_geom.h).
    uint32_t projection;     // PROJ_*
    double th;               // fisheye: half of vfov in radians, (vfov * (PI / 180)) / 2, formed on the host
    double focal_length;
    double fw, fh;           // width and height as doubles (converted on the host: see generate_ray)
    double forward[3], right[3], up[3];   // Camera::init's basis (pt_camera_init)
    // the shutter (pt_scene_set_shutter): a camera ray's time is shutter_open + shutter_span * u. Read by the MOT forms of K1 / K3 only.
    double shutter_open, shutter_span;
};
enum Projection : uint32_t { PROJ_PERSPECTIVE = 0, PROJ_ORTHOGRAPHIC = 1, PROJ_FISHEYE = 2, PROJ_PANORAMA = 3 };

// Environment importance sampling (pt_scene_set_env_sampling): the f64 tables of the camera's environment map,
// built by pt_envmap.hip, and the mixture weight. A separate kernel argument of k_shade's ENV forms and of k_env_probe — CamD and
// SceneD keep their layouts. col: H rows of W + 1 prefix sums of the texel weights w_ij (col[j*(W+1)] = 0, col[j*(W+1)+W] = R_j);
// row: H + 1 prefix sums of the row totals (row[0] = 0, row[H] = z).
struct EnvTabD {
    const double* col;
    const double* row;
    double z, f;
    uint32_t w, h;
};

struct SceneD {
    const BvhNode* nodes;
    const Entry* entries;
    const PrimRef* prims;
    const SphereD* spheres;
    const QuadD* quads;
    const TriD* tris;
    const TriAttr* tri_attr;     // parallel to tris when any mesh has normals/uvs, else null
    const uint32_t* tri_gid;     // BLAS-order triangle -> face index inside its mesh; global id = Entry::first_prim + that (a mesh may be placed several times)
    const InstD* insts;
    const TexD* tex;
    const MatD* mats;
    const uint8_t* atlas;
    const float* atlas_f;        // f32 RGB texels of the TEX_IMAGE_F32 textures
    const uint32_t* lights;      // entry indices of the lights list
    uint32_t tlas_root;          // child reference of the top-level root
    float tlas_extent;           // max |coordinate| of the top-level BVH boxes
    uint32_t n_entries, n_prims, n_lights;
    const CuboidBox* cuboid_box; // parallel to entry_box (cuboid records only)
    const EntryBox* entry_box;   // the flat top level's walk list: one record per entry, NON-MESH entries first (each group in entry order)
    uint32_t tlas_flat;          // n_entries <= TLAS_FLAT_MAX: K2 walks the entry list instead of the top-level tree
    uint32_t flat_pairs;         // tlas_flat and the scene has cuboids: the batch K2 runs its (ray, primitive) pair passes
    const GridD* grids;          // grid-density media (MatD::p[6] - 1 indexes it); read by k_shade's HET forms and the medium probe only
    const float* grid_vals;      // their f32 samples, one array (GridD::ofs)
    const double* light_cdf;     // exact light sampling (pt_scene_set_light_sampling): per light mesh of n faces the n + 1 running
                                 // area sums C[0] = 0 .. C[n] = A in face order, at Entry::pad[0]; read by k_shade's LSE forms and the light probe only
    const InstMotionD* inst_motion;   // parallel to insts, null when no instance moves; read by the MOT forms of K2 / K3 and the probes only
    const PunctualD* punctual;   // the punctual lights of the last build, null when there are none; read by the PLT forms of K3 and the probe only
    uint32_t n_punctual;
    double punctual_f;           // pt_scene_set_punctual_fraction: the selector's share of the punctual branch
    const double* punctual_cdf;  // the light grid's table of the last build, null when the grid is not in effect: the PLT and light-shaft
    PunctualGridD punctual_grid; // forms of K3 branch on it at run time; nothing else reads either
};
static_assert(sizeof(SceneD) <= 512, "SceneD travels by value: with CamD, PoolD and the rest of k_shade's arguments it stays far below the 4 KiB of kernel arguments");
constexpr int LIGHT_STACK = 24;          // LDS entries per lane of the LSE forms' all-hits mesh walk (pt_dev_lights.h): the deepest light mesh tree they take
constexpr uint32_t TLAS_FLAT_MAX = 24;   // round 1 (vector loads): 8-10 entries -26 % / -7 % K2 time, 17 entries (scene 5) +20 % -> limit 12;
                                          // round 2 (scalar loads, ldu): 17 entries -20 % -> limit raised

// ---- path pool (one slot per resident path) --------------------------------------------
// Two work-assignment modes:
//  static  (slots_per_pixel = k >= 1): slot s owns pixel (s % n_pixels) and renders samples
//          spp_begin + (s / n_pixels) + j*k into its own accumulator ax/ay/az; deterministic, and
//          for k = 1 exactly the reference's per-pixel sample order (camera.rs:106-108).
//  dynamic (default): a finished path pulls the next (pixel, sample) work item from one global
//          counter — wave-aggregated: ballot + popcount + one atomic per wave — so every lane
//          stays busy until the frame's sample budget is exhausted; radiance is added to the
//          frame accumulator with hardware f64 atomics. Work items are ordered sample-major and,
//          inside a sample, by 8x8 PIXEL TILES (item % (tiles*64) -> tile, pixel in tile), so that
//          the 64 lanes of a wave start on one compact tile: primary rays — half of all segments
//          in scene 6 — stay coherent in traversal and in material. Items that fall outside a
//          ragged image edge are skipped (slot state SLOT_IDLE for one iteration).
constexpr uint32_t HIT_NONE = 0xFFFFFFFFu;
// PoolD::hit_prim — what K2 hands to K3, one word per slot: the closest primitive's global id in bits 0..27 (all ones:
// nothing hit) and in bits 28..31 the CLASS k_shade sorts the slot by, so that K3's classification is ONE coalesced
// load per slot instead of a chain of three dependent ones (state -> id -> PrimRef): 0 miss, 1 + MatKind of the hit
// primitive's material, then idle and dead slots (K2 reads the slot state anyway).
constexpr uint32_t HIT_ID_MASK = 0x0FFFFFFFu, HIT_CLASS_SHIFT = 28;
constexpr uint32_t HIT_SLOT_IDLE = 0xFFFFFFFEu, HIT_SLOT_DEAD = 0xFFFFFFFDu;   // K2-internal sentinels next to HIT_NONE
constexpr uint32_t SLOT_DEAD = 0xFFFFFFFFu;   // value of `bounce` for a finished slot
constexpr uint32_t SLOT_IDLE = 0xFFFFFFFEu;   // dynamic mode: drew an item outside the image, draws again next iteration
// Path state is kept as two records per slot (array of structures): k_shade visits slots in
// material-class order and k_extend2's mesh pass visits them compacted, i.e. both PERMUTED inside a
// window — with one array per field every wave touched 1/8 of many 128-B lines and the rest of each
// line had left the L2 before the wave that needed it came by (measured 2.6 GB of HBM traffic per
// k_shade launch for 1.1 GB of state). A record is read/written whole by its own lane (16 B at a time).
// K2 reads RayRec only; K3 reads and writes both: 96 B in, 96 B out per segment.
struct alignas(64) RayRec {                       // current ray (direction normalised) + RNG position of the path
    double ox, oy, oz, dx, dy, dz, time;
    uint32_t sample, draw;                        // sample index, RNG draw counter
};
// 32 B. Measured (round 2, -DPT_PATHREC_BYTES=64): padding the record to a whole 64-B sector and writing all of it —
// so that K3 never writes half sectors — made K3 6 % SLOWER (560 vs 525 ms per 1000-spp frame of scene 6): two more 16-B
// stores per slot cost more than the partial-sector writes do. The 64-B form stays behind the macro for that measurement.
#ifndef PT_PATHREC_BYTES
#define PT_PATHREC_BYTES 32
#endif
struct alignas(PT_PATHREC_BYTES) PathRec {
    double tx, ty, tz;                            // throughput
    uint32_t pixel, pad;                          // dynamic mode: pixel of the sample in flight; pad: the bounce word (number, and the medium: MEDIUM_SHIFT)
#if PT_PATHREC_BYTES == 64
    double reserved[4];
#endif
};
struct PoolD {
    RayRec* ray;
    PathRec* path;
    double *ax, *ay, *az;                         // static mode: sum over this slot's finished samples
    double *rx, *ry, *rz;                         // static mode: radiance of the sample in flight (camera.rs:172); the dynamic
                                                  // mode adds every contribution to the frame accumulator right away
    uint32_t* hit_prim;
    uint32_t* bounce;                             // bounce count, or SLOT_DEAD / SLOT_IDLE
    double* accum;                                // dynamic mode: frame accumulator (W*H*3 sums). accum_tiled: three CHANNEL PLANES of
                                                  // n_tile_pixels sums each, a plane in the order the work items are handed out — tile
                                                  // after tile, 64 pixels of an 8x8 tile consecutive (index = plane + tile*64 + (y&7)*8 + (x&7)):
                                                  // the lanes of a group that finish together mostly hold pixels of the same few tiles, so one
                                                  // global_atomic_add_f64 wave-instruction covers runs of consecutive 8-byte words — whole 64-byte
                                                  // memory-side atomic requests (MI355X_MICROARCH.md "Global float atomics": they execute at the
                                                  // memory side, one request per 64 B touched) — instead of 64 requests at a 24-byte stride.
                                                  // k_detile adds the planes to the caller's (y, x, c) accumulator once per render.
    double inv_width;                             // 1 / width (pixel -> row by one multiplication and an exact correction)
    uint32_t accum_tiled;
    unsigned long long total_work;                // dynamic mode: n_pixels * (spp_end - spp_begin)
    uint32_t n_slots, n_pixels, k;                // k = slots per pixel (static mode)
    uint32_t spp_begin, spp_end;
    uint32_t dynamic, n_alloc;                    // n_alloc: slots rounded up to a multiple of 64
    uint32_t defer_regen, compact;                   // dynamic mode: a path that ends ON A SURFACE (roulette, sampler, depth) parks its slot
                                                  // as SLOT_IDLE; it is refilled next iteration among the idle slots (k_shade)
    uint32_t width, height, tiles_x, n_tile_pixels;   // dynamic mode: 8x8 tiling, n_tile_pixels = tiles_x*tiles_y*64
    // The sky pass (pt_k_sky.hip) is on: the work items cover the ACTIVE tiles only, n_work_pixels = 64 x their number, and
    // work_to_pixel maps an item's active-tile index through the tile map — u32 tile indices that lie BEHIND the three planes of the tiled
    // accumulator (pool_tile_map). 0: the pass is off, an item's tile is its index. The word fills what was padding and the map has no
    // pointer of its own, so that PoolD keeps its size and every field its offset: K2's code does not change by a byte.
    uint32_t n_work_pixels;
    // pixel-list renders (pt_render_pixels, pt_render_adaptive; the kernels' LIST = true forms only): n_list row-major pixel ids
    // in TILED-index order, so that consecutive work items / slots are neighbouring pixels as in a whole-frame render. Dynamic mode:
    // work item w = (pixel list[w mod n_list], sample spp_begin + w / n_list); static mode: slot s owns pixel list[s mod n_list].
    // list_store: k_resolve / k_detile store the listed pixels' sums instead of adding them (device accumulator + overwrite).
    const uint32_t* list;
    uint32_t n_list, list_store;
    // Shading-order output (dynamic mode, sorted whole-frame k_shade; PoolD::reorder): k_shade reads a window's records where they
    // are and writes every surviving path, its regenerated camera ray or its parked slot to ray_out / path_out / bounce_out at the
    // window's base + the lane's position in the window's SORTED order (64 * group + lane), and the state of every other position
    // of the window as SLOT_DEAD. The host swaps the two areas after each k_shade launch, so K2 and the next K3 read what K3 wrote:
    // a K2 chunk of 64 consecutive slots is one K3 group — a tile's camera rays in pixel order, or 64 paths of one material class.
    // reorder = 0 (static mode, pixel lists, PT_POOL_IN_PLACE): the out pointers equal ray / path / bounce and K3 writes in place.
    RayRec* ray_out;
    PathRec* path_out;
    uint32_t* bounce_out;
    uint32_t reorder;
    uint32_t init_perm;                           // experiment (PT_INIT_SHUFFLE): k_init gives slot s the item pi(s) inside each 8192-slot granule, 0 = identity
};

static_assert(sizeof(PoolD) == 216 && offsetof(PoolD, list) == 168 && offsetof(PoolD, n_work_pixels) == 164, "PoolD's layout is part of K2's code");

// The short-path pass (pt_k_short.hip): the samples of its tiles it could not finish — the HARD samples — are work items of
// the wavefront behind the tile items: item n_work_pixels x spp + i is entry i of the hard list. This record says where the list is; it lies
// behind the sky pass's tile map (pt_k_common.h pool_short_hdr), so PoolD stays what it is. An entry packs (ordinal of the tile in the
// short-tile list) << (6 + sample_bits) | (pixel in tile) << sample_bits | (sample - spp_begin), in 4 bytes where that fits (wide = 0) and
// in 8 where it does not; the host decides per render. The host writes the record whenever the sky pass is on (n_hard = 0: no such items).
struct ShortHdrD {
    const void* hard;
    const uint32_t* short_list;
    uint32_t wide, sample_bits;
    unsigned long long n_hard;
};
// k_short's own arguments: the short tiles (in tile order) and how their samples are cut into waves; the global ids of the shadeable
// primitives; the hard list, its format (ShortHdrD), its capacity in entries and three device words: [0] counts what was appended, [1] the
// samples the pass finished, [2] their segments (the render's counters are started after the pass: the host adds these to them).
struct ShortArgsD {
    const uint32_t* short_list;
    uint32_t n_short, chunk, n_chunks;
    const uint32_t* shade_prims;
    uint32_t n_shade;
    void* hard;
    unsigned long long* n_hard;
    unsigned long long cap;
    uint32_t wide, sample_bits;
    uint32_t* pilot;      // not null: the counting form runs (k_short<true>) and writes {finished, seen} at pilot[2 * tile]
    uint32_t walk_cap;    // the miss proof's stack budget in entries per lane (<= SHORT_WALK_STACK)
    uint32_t defer;       // the bounces' miss proofs run in dense passes (0: where the ray enters the box, PT_SHORT_DEFER=0)
    // DESIGN.md §23.3. reach: per tile of the frame, the entries a camera ray of the tile may enter, bit k = SceneD::entry_box[k] (k_sky_classify;
    // null: all ones, PT_SHORT_REACH=0). shade_at: parallel to shade_prims, the entry's place k in entry_box, | SHADE_AT_SELF_OK for a quad a
    // bounce that left it need not test again (null bit: it tests it; PT_SHORT_SELF=0 clears them all). direct: a tile whose mask names one
    // shadeable entry rebuilds the hit without the top level's loop (0: PT_SHORT_DIRECT=0)
    const uint32_t* reach;
    const uint32_t* shade_at;
    uint32_t direct;
};
constexpr uint32_t SHADE_AT_SELF_OK = 0x100u;
// ShortArgsD::n_hard's device words: the three above, [3] the deferred records walked, [4] the passes that walked them (the render's pass, not
// the pilot's), [5] the tiles rendered by the direct hit; a diagnostic build (-DPT_STAMPS) sums k_short's wave cycles and walk counts from word SHORT_PROF_AT on (pt_k_short.hip).
constexpr uint32_t SHORT_WORDS = 40, SHORT_PROF_AT = 8;
constexpr uint32_t SHORT_WALK_STACK = 16;   // the miss proof's stack per lane in LDS (16 KB per block)
constexpr uint32_t SHORT_YIELD_BINS = 17;   // pilot yields in sixteenths: bin = floor(16 finished / seen), 0 .. 16

// The work counter of the dynamic mode is SHARDED: one word saturates at ~88 dequeues/us on this
// chip (MI355X_MICROARCH.md, row "dequeue") and a frame needs one dequeue per wave per iteration
// (65k per launch at 4M resident paths), which alone would cost ~0.75 ms per launch. Shard s hands
// out the work items w with w % WORK_SHARDS == s; a block always uses shard blockIdx.x % WORK_SHARDS.
constexpr uint32_t WORK_SHARDS = 64;
#ifdef PT_STAMPS
constexpr int PROF_COLS = 14;   // diagnostic build (-DPT_STAMPS): columns of the per-class profile
#else
constexpr int PROF_COLS = 12;   // (the last two — single-primitive groups — exist in the diagnostic build only)
#endif
struct CountersD {
    unsigned long long alive;        // slots still rendering
    unsigned long long segments;     // extend() calls on live paths
    unsigned long long samples;      // finished samples
    // window queues of k_extend2 / k_shade<sort>: blocks draw the next window of the pool from these instead
    // of striding over it (window costs differ by an order of magnitude between sky and mesh tiles). Each
    // kernel zeroes the OTHER kernel's queue; the two alternate on one stream.
    unsigned long long win_extend, win_shade;
    // k_extend2's rounds (pt_k2_extend.h "rounds of a window"): the mid-window rounds it ran, and the rays phase A walked itself because the
    // candidate list was full. In what was padding: no field moves.
    unsigned long long k2_split_windows, k2_overflow_rays;
    unsigned long long pad[9];
    // diagnostic builds only (-DPT_STAMPS, tools/build_variant.sh): wave-cycle sums per k_shade class
    // [class][0 groups, 1 record-load wait, 2 body, 3 work dequeue, 4 regeneration + stores, 5 whole, .., 12 groups whose surface lanes hit one
    // primitive, 13 those whose primitive is no triangle], [N_CLASSES][..] = window phases
    unsigned long long prof[N_CLASSES + 1][PROF_COLS];
    struct alignas(128) Shard { unsigned long long next; unsigned long long pad[15]; } work[WORK_SHARDS];
};

}  // namespace pt
