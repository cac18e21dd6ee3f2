"""MI355X-native wavefront path tracer — Python binding of the C ABI (include/pt_amd.h).

This is the drop-in for ONE path of chiefchewie/thu-acg-f2024-path-tracer: the per-pixel
integrator behind ``Camera::render`` (src/camera.rs:79). The binding is ctypes over
``libpt_amd.so`` (hand-written HIP kernels for gfx950 + C++ host runtime); there is no CPU
fallback — importing works without a GPU (so the symbol table can be checked), creating a
:class:`Context` does not.

Because the directory name contains hyphens, import it with
``importlib.import_module("thu-acg-f2024-path-tracer_amd")``.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(_HERE)
# PT_AMD_LIB: A/B measurements of two builds of the library in one session (tools/ab_perf.sh); never a different backend
LIB_PATH = os.environ.get("PT_AMD_LIB") or os.path.join(_HERE, "libpt_amd.so")
ASSET_DIR = os.path.join(REPO_ROOT, "assets")


class PtError(RuntimeError):
    pass


class Camera(C.Structure):
    """The 12 public fields of the reference's ``Camera`` (src/camera.rs:23-36)."""

    _fields_ = [
        ("aspect_ratio", C.c_double),
        ("image_width", C.c_uint32),
        ("samples_per_pixel", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("env_is_map", C.c_uint32),
        ("vfov", C.c_double),
        ("look_from", C.c_double * 3),
        ("look_at", C.c_double * 3),
        ("vup", C.c_double * 3),
        ("blur_strength", C.c_double),
        ("focal_length", C.c_double),
        ("defocus_angle", C.c_double),
        ("env_color", C.c_double * 3),
        ("env_tex", C.c_int32),
        ("_pad", C.c_int32),
    ]


class RenderOpts(C.Structure):
    _fields_ = [
        ("slots_per_pixel", C.c_uint32),
        ("accum_on_device", C.c_uint32),
        ("profile", C.c_uint32),
        ("overwrite", C.c_uint32),
        ("stream", C.c_void_p),
    ]


class RenderStats(C.Structure):
    _fields_ = [
        ("samples", C.c_uint64),
        ("segments", C.c_uint64),
        ("iterations", C.c_uint64),
        ("n_slots", C.c_uint32),
        ("slots_per_pixel", C.c_uint32),
        ("ms_total", C.c_double),
        ("ms_extend", C.c_double),
        ("ms_shade", C.c_double),
        ("ms_other", C.c_double),
        ("launches_extend", C.c_uint64),
        ("launches_shade", C.c_uint64),
        ("extend_variant", C.c_uint32),
        ("shade_variant", C.c_uint32),
        ("blocks_extend", C.c_uint32),
        ("blocks_shade", C.c_uint32),
        ("compactions", C.c_uint32),
        ("n_alloc_end", C.c_uint32),
        ("k2_split_windows", C.c_uint64),
        ("k2_overflow_rays", C.c_uint64),
        ("short_direct_tiles", C.c_uint64),
        ("short_self_prims", C.c_uint64),
        ("short_walks", C.c_uint64),
        ("short_walk_passes", C.c_uint64),
        ("pilot_tiles", C.c_uint64),
        ("short_fallback", C.c_uint64),
        ("short_list_bytes", C.c_uint64),
        ("short_pixels", C.c_uint64),
        ("ms_pilot", C.c_double),
        ("short_tiles", C.c_uint64),
        ("short_samples", C.c_uint64),
        ("hard_samples", C.c_uint64),
        ("ms_short", C.c_double),
        ("sky_tiles", C.c_uint64),
        ("sky_samples", C.c_uint64),
        ("ms_sky", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AdaptiveOpts(C.Structure):
    _fields_ = [
        ("min_spp", C.c_uint32),
        ("max_spp", C.c_uint32),
        ("threshold", C.c_double),
        ("slots_per_pixel", C.c_uint32),
        ("profile", C.c_uint32),
        ("stream", C.c_void_p),
    ]


class DenoiseOpts(C.Structure):
    """pt_denoise_opts: a-trous levels and the two edge-stopping widths (include/pt_amd.h has the rule)."""

    _fields_ = [
        ("iterations", C.c_uint32),
        ("sigma_l", C.c_double),
        ("sigma_z", C.c_double),
    ]


TONEMAPS = {"reference": 0, "srgb": 1, "reinhard": 2, "aces": 3}   # pt_film_opts.tonemap


class FilmOpts(C.Structure):
    """pt_film_opts: exposure, tone curve and glare of the film stage (include/pt_amd.h has the rule). A fresh instance holds the defaults."""

    _fields_ = [
        ("exposure_ev", C.c_double),
        ("tonemap", C.c_uint32),
        ("white", C.c_double),
        ("bloom_strength", C.c_double),
        ("bloom_threshold", C.c_double),
        ("bloom_sigma", C.c_double),
        ("bloom_levels", C.c_uint32),
        ("on_device", C.c_uint32),
        ("stream", C.c_void_p),
    ]

    def __init__(self, exposure_ev=0.0, tonemap=0, white=4.0, bloom_strength=0.0, bloom_threshold=1.0, bloom_sigma=2.0, bloom_levels=5,
                 on_device=0, stream=None):
        super().__init__(exposure_ev, TONEMAPS.get(tonemap, tonemap), white, bloom_strength, bloom_threshold, bloom_sigma, bloom_levels,
                         on_device, stream)


class SkyOpts(C.Structure):
    """pt_sky_opts: the physical sky's sun direction, turbidity, ground, disc and scales (include/pt_amd.h has the rule). A fresh instance
    holds the defaults: the sun at the zenith, turbidity 3."""

    _fields_ = [
        ("sun_dir", C.c_double * 3),
        ("turbidity", C.c_double),
        ("ground_albedo", C.c_double * 3),
        ("sun_radius_deg", C.c_double),
        ("sun_scale", C.c_double),
        ("scale", C.c_double),
    ]

    def __init__(self, sun_dir=(0.0, 1.0, 0.0), turbidity=3.0, ground_albedo=(0.3, 0.3, 0.3), sun_radius_deg=0.2665, sun_scale=1.0, scale=0.04):
        if np.ndim(ground_albedo) == 0:
            ground_albedo = (ground_albedo,) * 3
        super().__init__(_d3(sun_dir), turbidity, _d3(ground_albedo), sun_radius_deg, sun_scale, scale)


TESS_WRAPS = {"clamp": 0, "repeat": 1}                          # pt_tess_opts.wrap
TESS_NORMALS = {"auto": 0, "keep": 1, "smooth": 2, "none": 3}   # pt_tess_opts.normals


class TessOpts(C.Structure):
    """pt_tess_opts: subdivision levels, the height image and how it displaces, which normals are written (include/pt_amd.h has the
    rule). A fresh instance holds the defaults: one level, no displacement. `height` is an (H, W) float32 image, row 0 at v = 1; the
    instance keeps it alive."""

    _fields_ = [
        ("levels", C.c_uint32),
        ("height_w", C.c_uint32),
        ("height_h", C.c_uint32),
        ("height", C.c_void_p),
        ("scale", C.c_double),
        ("midlevel", C.c_double),
        ("wrap", C.c_int),
        ("normals", C.c_int),
    ]

    def __init__(self, levels=1, height=None, scale=1.0, midlevel=0.5, wrap="clamp", normals="auto"):
        wrap = TESS_WRAPS.get(wrap, wrap)
        normals = TESS_NORMALS.get(normals, normals)
        if height is None:
            super().__init__(levels, 0, 0, None, scale, midlevel, wrap, normals)
        else:
            self._height = np.ascontiguousarray(height, dtype=np.float32)
            if self._height.ndim != 2:
                raise ValueError("height must be an (H, W) image")
            super().__init__(levels, self._height.shape[1], self._height.shape[0], self._height.ctypes.data, scale, midlevel, wrap, normals)


SUBDIV_NORMALS = {"smooth": 0, "none": 1}   # pt_subdiv_opts.normals


def _cos_deg(deg, default):
    """The cosine pt_subdiv_opts wants for an angle in degrees (None: `default`, the value that switches the test off)"""
    return default if deg is None else math.cos(math.radians(float(deg)))


class SubdivOpts(C.Structure):
    """pt_subdiv_opts: Loop subdivision levels, the two angle thresholds as cosines, limit projection, which normals are written
    (include/pt_amd.h has the rule). A fresh instance holds the defaults: one level, no angle test, no projection, smooth normals."""

    _fields_ = [
        ("levels", C.c_uint32),
        ("crease_cos", C.c_double),
        ("corner_cos", C.c_double),
        ("limit", C.c_int),
        ("normals", C.c_int),
    ]

    def __init__(self, levels=1, crease_cos=-2.0, corner_cos=2.0, limit=0, normals="smooth"):
        super().__init__(levels, crease_cos, corner_cos, int(limit), SUBDIV_NORMALS.get(normals, normals))


ISO_NORMALS = {"gradient": 0, "smooth": 1, "none": 2}   # pt_iso_opts.normals


class IsoOpts(C.Structure):
    """pt_iso_opts: the level, whether the surface is closed by a layer of `outside` samples, which normals are written
    (include/pt_amd.h has the rule). A fresh instance holds the defaults: level 0.5, open, gradient normals."""

    _fields_ = [
        ("iso", C.c_double),
        ("closed", C.c_int),
        ("outside", C.c_float),
        ("normals", C.c_int),
    ]

    def __init__(self, iso=0.5, closed=0, outside=0.0, normals="gradient"):
        super().__init__(iso, int(closed), outside, ISO_NORMALS.get(normals, normals))


SDF_WHAT = {"depth": 0, "distance": 1, "occupancy": 2, "density": 3}   # pt_sdf_opts.what
SDF_FILL = {"nonzero": 0, "odd": 1}                                    # pt_sdf_opts.fill


class SdfOpts(C.Structure):
    """pt_sdf_opts: what is written (depth, positive inside / distance / occupancy / density), which winding numbers are inside, the
    band distances are capped at and the density's ramp (include/pt_amd.h has the rule). A fresh instance holds the defaults."""

    _fields_ = [
        ("what", C.c_int),
        ("fill", C.c_int),
        ("negate", C.c_int),
        ("band", C.c_double),
        ("ramp", C.c_double),
    ]

    def __init__(self, what="depth", fill="nonzero", negate=False, band=0.0, ramp=None):
        super().__init__(SDF_WHAT.get(what, what), SDF_FILL.get(fill, fill), int(negate), band, 0.0 if ramp is None else ramp)


SIMPLIFY_MODES = {"weld": 0, "cluster": 1}       # pt_simplify_opts.mode
SIMPLIFY_PLACEMENTS = {"quadric": 0, "mean": 1}   # pt_simplify_opts.placement


class SimplifyOpts(C.Structure):
    """pt_simplify_opts: weld or cluster, the cell (or the cells along the longest extent), where a cluster's vertex is placed, whether
    coincident triangles cancel, which normals are written (include/pt_amd.h has the rule). A fresh instance holds the defaults:
    clustering at 64 cells, quadric placement with reg 1e-3, dedup, smooth normals."""

    _fields_ = [
        ("mode", C.c_int),
        ("cell", C.c_double),
        ("grid_n", C.c_uint32),
        ("placement", C.c_int),
        ("reg", C.c_double),
        ("dedup", C.c_int),
        ("normals", C.c_int),
    ]

    def __init__(self, mode="cluster", cell=0.0, grid_n=64, placement="quadric", reg=1e-3, dedup=True, normals="smooth"):
        super().__init__(SIMPLIFY_MODES.get(mode, mode), cell, grid_n, SIMPLIFY_PLACEMENTS.get(placement, placement), reg, int(dedup),
                         SUBDIV_NORMALS.get(normals, normals))


# every symbol include/pt_amd.h declares (the not-gpu test checks the library exports them all)
ABI_SYMBOLS = [
    "pt_last_error", "pt_set_error_message", "pt_ctx_create", "pt_ctx_destroy", "pt_device_name",
    "pt_scene_create", "pt_scene_destroy", "pt_scene_ctx",
    "pt_tex_solid_rgb", "pt_tex_solid_f", "pt_tex_checker", "pt_tex_image_rgb8", "pt_tex_image_rgbf32", "pt_scene_set_float_hdr", "pt_scene_float_hdr",
    "pt_scene_set_env_sampling", "pt_scene_env_sampling", "pt_env_probe",
    "pt_scene_set_sampler", "pt_scene_sampler", "pt_sampler_probe",
    "pt_mat_diffuse", "pt_mat_metal", "pt_mat_glass", "pt_mat_principled", "pt_mat_light", "pt_mat_mix", "pt_mat_sheen", "pt_mat_clearcoat",
    "pt_sphere", "pt_quad", "pt_cuboid", "pt_mesh", "pt_instance",
    "pt_world_add_object", "pt_world_add_light", "pt_world_build", "pt_world_prim_count",
    "pt_world_set_device_bvh_threshold", "pt_world_device_bvh_info",
    "pt_load_obj", "pt_load_obj_single_index", "pt_load_hdr_rgb8", "pt_load_hdr_rgbf32", "pt_load_png_rgb8", "pt_load_jpeg_rgb8", "pt_free", "pt_register_image", "pt_find_registered_image", "pt_save_png",
    "pt_build_scene", "pt_camera_init", "pt_render", "pt_resolve_u8", "pt_intersect", "pt_math_probe",
    "pt_shard_range", "pt_comm_create", "pt_comm_destroy", "pt_comm_rank", "pt_comm_world", "pt_comm_barrier", "pt_comm_allreduce_f64",
    "pt_bootstrap_exchange", "pt_render_multi",
    "pt_render_pixels", "pt_adaptive_schedule", "pt_render_adaptive", "pt_resolve_u8_counts",
    "pt_render_aovs", "pt_denoise",
    "pt_film_opts_check", "pt_film_develop", "pt_save_hdr", "pt_save_pfm",
    "pt_mat_medium", "pt_scene_set_camera_medium", "pt_scene_camera_medium", "pt_medium_probe",
    "pt_mat_medium_grid",
    "pt_mat_medium_tinted", "pt_mat_glass_set_interior", "pt_mat_glass_interior",
    "pt_scene_set_light_sampling", "pt_scene_light_sampling", "pt_light_probe",
    "pt_mat_glass_set_dispersion", "pt_mat_glass_dispersion", "pt_dispersion_probe",
    "pt_scene_set_projection", "pt_scene_projection", "pt_camera_probe",
    "pt_instance_moving", "pt_scene_set_shutter", "pt_scene_shutter", "pt_scene_motion", "pt_motion_pose", "pt_motion_swept_box", "pt_world_entry_box",
    "pt_sky_tiles", "pt_short_tiles", "pt_tile_reach",
    "pt_light_point", "pt_light_spot", "pt_light_directional", "pt_scene_clear_punctual_lights", "pt_scene_punctual_count", "pt_scene_punctual_light",
    "pt_scene_set_punctual_fraction", "pt_scene_punctual_fraction", "pt_punctual_probe", "pt_punctual_eval", "pt_scene_set_punctual_media", "pt_scene_punctual_media",
    "pt_scene_set_punctual_selection", "pt_scene_punctual_selection", "pt_scene_set_punctual_grid", "pt_scene_punctual_grid", "pt_punctual_grid_row", "pt_punctual_grid_select",
    "pt_sky_opts_default", "pt_sky_opts_check", "pt_sky_eval", "pt_sky_sun_irradiance", "pt_sky_probe", "pt_sky_bake", "pt_tex_sky",
    "pt_tess_opts_default", "pt_mesh_tessellate", "pt_mesh_tessellate_host", "pt_mesh_grid", "pt_height_from_rgb8",
    "pt_subdiv_opts_default", "pt_mesh_subdivide", "pt_mesh_subdivide_host",
    "pt_iso_opts_default", "pt_mesh_isosurface", "pt_mesh_isosurface_host",
    "pt_sdf_opts_default", "pt_mesh_sdf", "pt_mesh_sdf_host", "pt_mesh_fit_grid",
    "pt_simplify_opts_default", "pt_mesh_simplify", "pt_mesh_simplify_host",
]


def _load():
    if not os.path.exists(LIB_PATH):
        raise PtError(
            f"{LIB_PATH} is missing: build it with `make -C {_HERE}` (or __graft_entry__.build()). "
            "There is no Python/CPU fallback for the render path."
        )
    lib = C.CDLL(LIB_PATH)
    lib.pt_last_error.restype = C.c_char_p
    lib.pt_scene_create.restype = C.c_void_p
    lib.pt_scene_create.argtypes = [C.c_void_p]
    lib.pt_scene_destroy.argtypes = [C.c_void_p]
    lib.pt_scene_destroy.restype = None
    lib.pt_scene_ctx.restype = C.c_void_p
    lib.pt_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.pt_ctx_destroy.argtypes = [C.c_void_p]
    lib.pt_ctx_destroy.restype = None
    lib.pt_device_name.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32]
    d3 = C.POINTER(C.c_double)
    lib.pt_tex_solid_rgb.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double]
    lib.pt_tex_solid_f.argtypes = [C.c_void_p, C.c_double]
    lib.pt_tex_checker.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int]
    lib.pt_tex_image_rgb8.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.pt_tex_image_rgbf32.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.pt_scene_set_float_hdr.argtypes = [C.c_void_p, C.c_int]
    lib.pt_scene_float_hdr.argtypes = [C.c_void_p]
    lib.pt_scene_set_env_sampling.argtypes = [C.c_void_p, C.c_double]
    lib.pt_scene_env_sampling.argtypes = [C.c_void_p]
    lib.pt_scene_env_sampling.restype = C.c_double
    if hasattr(lib, "pt_scene_set_sampler"):       # (absent from an older build in an A/B run: PT_AMD_LIB)
        lib.pt_scene_set_sampler.argtypes = [C.c_void_p, C.c_int]
        lib.pt_scene_sampler.argtypes = [C.c_void_p]
        lib.pt_sampler_probe.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    if hasattr(lib, "pt_mat_medium"):              # (absent from an older build in an A/B run: PT_AMD_LIB)
        lib.pt_mat_medium.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]
        lib.pt_scene_set_camera_medium.argtypes = [C.c_void_p, C.c_int]
        lib.pt_scene_camera_medium.argtypes = [C.c_void_p]
        lib.pt_medium_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    if hasattr(lib, "pt_mat_medium_grid"):         # (absent from an older build in an A/B run: PT_AMD_LIB)
        lib.pt_mat_medium_grid.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(lib, "pt_mat_medium_tinted"):       # (absent from an older build in an A/B run: PT_AMD_LIB)
        lib.pt_mat_medium_tinted.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]
        lib.pt_mat_glass_set_interior.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.pt_mat_glass_interior.argtypes = [C.c_void_p, C.c_int]
    if hasattr(lib, "pt_scene_set_light_sampling"):   # (absent from an older build in an A/B run: PT_AMD_LIB)
        lib.pt_scene_set_light_sampling.argtypes = [C.c_void_p, C.c_int]
        lib.pt_scene_light_sampling.argtypes = [C.c_void_p]
        lib.pt_light_probe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    if hasattr(lib, "pt_mat_glass_set_dispersion"):   # (absent from an older build in an A/B run: PT_AMD_LIB)
        lib.pt_mat_glass_set_dispersion.argtypes = [C.c_void_p, C.c_int, C.c_double]
        lib.pt_mat_glass_dispersion.argtypes = [C.c_void_p, C.c_int]
        lib.pt_mat_glass_dispersion.restype = C.c_double
        lib.pt_dispersion_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
    if hasattr(lib, "pt_scene_set_projection"):   # (absent from an older build in an A/B run: PT_AMD_LIB)
        lib.pt_scene_set_projection.argtypes = [C.c_void_p, C.c_int]
        lib.pt_scene_projection.argtypes = [C.c_void_p]
        lib.pt_camera_probe.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
    if hasattr(lib, "pt_instance_moving"):   # (absent from an older build in an A/B run: PT_AMD_LIB)
        lib.pt_instance_moving.argtypes = [C.c_void_p, C.c_int, d3, C.c_double, C.c_double, d3, d3]
        lib.pt_scene_set_shutter.argtypes = [C.c_void_p, C.c_double, C.c_double]
        lib.pt_scene_shutter.argtypes = [C.c_void_p, d3]
        lib.pt_scene_motion.argtypes = [C.c_void_p]
        lib.pt_motion_pose.argtypes = [d3, C.c_double, C.c_double, d3, d3, C.c_double, d3]
        lib.pt_motion_swept_box.argtypes = [d3, d3, C.c_double, C.c_double, d3, d3, d3]
        lib.pt_world_entry_box.argtypes = [C.c_void_p, C.c_uint32, d3]
    if hasattr(lib, "pt_light_point"):   # (absent from an older build in an A/B run: PT_AMD_LIB)
        lib.pt_light_point.argtypes = [C.c_void_p, d3, d3]
        lib.pt_light_spot.argtypes = [C.c_void_p, d3, d3, C.c_double, C.c_double, d3]
        lib.pt_light_directional.argtypes = [C.c_void_p, d3, d3]
        lib.pt_scene_clear_punctual_lights.argtypes = [C.c_void_p]
        lib.pt_scene_punctual_count.argtypes = [C.c_void_p]
        lib.pt_scene_punctual_light.argtypes = [C.c_void_p, C.c_int, d3]
        lib.pt_scene_set_punctual_fraction.argtypes = [C.c_void_p, C.c_double]
        lib.pt_scene_punctual_fraction.argtypes = [C.c_void_p]
        lib.pt_scene_punctual_fraction.restype = C.c_double
        lib.pt_punctual_probe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.pt_punctual_eval.argtypes = [d3, d3, d3]
    if hasattr(lib, "pt_scene_set_punctual_media"):
        lib.pt_scene_set_punctual_media.argtypes = [C.c_void_p, C.c_int]
        lib.pt_scene_punctual_media.argtypes = [C.c_void_p]
    if hasattr(lib, "pt_scene_set_punctual_selection"):
        lib.pt_scene_set_punctual_selection.argtypes = [C.c_void_p, C.c_int]
        lib.pt_scene_punctual_selection.argtypes = [C.c_void_p]
        lib.pt_scene_set_punctual_grid.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.pt_scene_punctual_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.pt_punctual_grid_row.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.pt_punctual_grid_select.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    if hasattr(lib, "pt_sky_tiles"):
        lib.pt_sky_tiles.argtypes = [C.POINTER(Camera), C.c_uint32, C.c_void_p, C.c_void_p]
    if hasattr(lib, "pt_short_tiles"):             # (absent from an older build in an A/B run: PT_AMD_LIB)
        lib.pt_short_tiles.argtypes = [C.POINTER(Camera), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "pt_tile_reach"):
        lib.pt_tile_reach.argtypes = [C.POINTER(Camera), C.c_uint32, C.c_void_p, C.c_void_p]
    lib.pt_load_hdr_rgbf32.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.pt_mat_diffuse.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.pt_mat_metal.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.pt_mat_glass.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.pt_mat_principled.argtypes = [C.c_void_p, C.c_int, d3]
    lib.pt_mat_light.argtypes = [C.c_void_p, C.c_int]
    lib.pt_mat_mix.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int]
    lib.pt_mat_sheen.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double]
    lib.pt_mat_clearcoat.argtypes = [C.c_void_p, C.c_double]
    lib.pt_sphere.argtypes = [C.c_void_p, C.c_double, d3, d3, C.c_int]
    lib.pt_quad.argtypes = [C.c_void_p, d3, d3, d3, C.c_int]
    lib.pt_cuboid.argtypes = [C.c_void_p, d3, d3, C.c_int]
    lib.pt_mesh.argtypes = [C.c_void_p, C.c_double, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                            C.c_uint32, C.c_void_p, C.c_int]
    lib.pt_instance.argtypes = [C.c_void_p, C.c_int, d3, C.c_double, d3]
    lib.pt_world_add_object.argtypes = [C.c_void_p, C.c_int]
    lib.pt_world_add_light.argtypes = [C.c_void_p, C.c_int]
    lib.pt_world_build.argtypes = [C.c_void_p]
    lib.pt_world_prim_count.argtypes = [C.c_void_p]
    lib.pt_world_prim_count.restype = C.c_uint32
    if hasattr(lib, "pt_world_set_device_bvh_threshold"):
        lib.pt_world_set_device_bvh_threshold.argtypes = [C.c_void_p, C.c_uint32]
        lib.pt_world_device_bvh_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.pt_register_image.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.pt_find_registered_image.argtypes = [C.c_void_p, C.c_char_p]
    lib.pt_save_png.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.pt_build_scene.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, C.POINTER(Camera)]
    lib.pt_camera_init.argtypes = [C.POINTER(Camera), d3, C.POINTER(C.c_uint32)]
    lib.pt_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p,
                              C.POINTER(RenderOpts), C.POINTER(RenderStats)]
    lib.pt_resolve_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.pt_intersect.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.pt_math_probe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.pt_env_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.pt_load_obj.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint32)),
                                C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint32)]
    lib.pt_load_hdr_rgb8.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    if hasattr(lib, "pt_load_jpeg_rgb8"):
        lib.pt_load_jpeg_rgb8.argtypes = lib.pt_load_hdr_rgb8.argtypes
    if hasattr(lib, "pt_load_png_rgb8"):
        lib.pt_load_png_rgb8.argtypes = lib.pt_load_hdr_rgb8.argtypes
        fp, up = C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint32)
        lib.pt_load_obj_single_index.argtypes = [C.c_char_p, fp, up, C.POINTER(C.POINTER(C.c_uint32)), up, fp, up, fp, up]
    lib.pt_free.argtypes = [C.c_void_p]
    lib.pt_free.restype = None
    if hasattr(lib, "pt_render_pixels"):
        lib.pt_render_pixels.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                         C.POINTER(RenderOpts), C.POINTER(RenderStats)]
        lib.pt_adaptive_schedule.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
        lib.pt_render_adaptive.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint64, C.POINTER(AdaptiveOpts), C.c_void_p, C.c_void_p,
                                           C.POINTER(RenderStats)]
        lib.pt_resolve_u8_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    if hasattr(lib, "pt_render_aovs"):
        lib.pt_render_aovs.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RenderOpts)]
        lib.pt_denoise.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                   C.POINTER(DenoiseOpts), C.c_void_p]
    if hasattr(lib, "pt_film_develop"):            # (absent from an older build in an A/B run: PT_AMD_LIB)
        lib.pt_film_develop.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(FilmOpts), C.c_void_p, C.c_void_p]
        lib.pt_film_opts_check.argtypes = [C.POINTER(FilmOpts)]
        lib.pt_save_hdr.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.pt_save_pfm.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]
    if hasattr(lib, "pt_sky_bake"):                # (absent from an older build in an A/B run: PT_AMD_LIB)
        lib.pt_sky_opts_default.argtypes = [C.POINTER(SkyOpts)]
        lib.pt_sky_opts_check.argtypes = [C.POINTER(SkyOpts)]
        lib.pt_sky_eval.argtypes = [C.POINTER(SkyOpts), C.c_void_p, C.c_uint32, C.c_void_p]
        lib.pt_sky_sun_irradiance.argtypes = [C.POINTER(SkyOpts), d3]
        lib.pt_sky_probe.argtypes = [C.c_void_p, C.POINTER(SkyOpts), C.c_void_p, C.c_uint32, C.c_void_p]
        lib.pt_sky_bake.argtypes = [C.c_void_p, C.POINTER(SkyOpts), C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]
        lib.pt_tex_sky.argtypes = [C.c_void_p, C.POINTER(SkyOpts), C.c_uint32, C.c_uint32]
    if hasattr(lib, "pt_mesh_tessellate"):         # (absent from an older build in an A/B run: PT_AMD_LIB)
        fpp, upp, up = C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)
        mesh_in = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        mesh_out = [fpp, up, upp, up, fpp, fpp]
        lib.pt_tess_opts_default.argtypes = [C.POINTER(TessOpts)]
        lib.pt_mesh_tessellate.argtypes = [C.c_void_p, C.POINTER(TessOpts)] + mesh_in + mesh_out
        lib.pt_mesh_tessellate_host.argtypes = [C.POINTER(TessOpts)] + mesh_in + mesh_out
        lib.pt_mesh_grid.argtypes = [d3, d3, d3, C.c_uint32, C.c_uint32] + mesh_out
        lib.pt_height_from_rgb8.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    if hasattr(lib, "pt_mesh_subdivide"):          # (absent from an older build in an A/B run: PT_AMD_LIB)
        fpp, upp, up = C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)
        sub_args = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, fpp, up, upp, up, fpp, fpp, C.POINTER(C.POINTER(C.c_uint8))]
        lib.pt_subdiv_opts_default.argtypes = [C.POINTER(SubdivOpts)]
        lib.pt_mesh_subdivide.argtypes = [C.c_void_p, C.POINTER(SubdivOpts)] + sub_args
        lib.pt_mesh_subdivide_host.argtypes = [C.POINTER(SubdivOpts)] + sub_args
    if hasattr(lib, "pt_mesh_isosurface"):         # (absent from an older build in an A/B run: PT_AMD_LIB)
        fpp, upp, up = C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)
        iso_args = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, fpp, up, upp, up, fpp]
        lib.pt_iso_opts_default.argtypes = [C.POINTER(IsoOpts)]
        lib.pt_mesh_isosurface.argtypes = [C.c_void_p, C.POINTER(IsoOpts)] + iso_args
        lib.pt_mesh_isosurface_host.argtypes = [C.POINTER(IsoOpts)] + iso_args
    if hasattr(lib, "pt_mesh_sdf"):                # (absent from an older build in an A/B run: PT_AMD_LIB)
        sdf_args = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.pt_sdf_opts_default.argtypes = [C.POINTER(SdfOpts)]
        lib.pt_mesh_sdf.argtypes = [C.c_void_p, C.POINTER(SdfOpts)] + sdf_args
        lib.pt_mesh_sdf_host.argtypes = [C.POINTER(SdfOpts)] + sdf_args
        lib.pt_mesh_fit_grid.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "pt_mesh_simplify"):           # (absent from an older build in an A/B run: PT_AMD_LIB)
        fpp, upp, up = C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)
        simp_args = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, fpp, up, upp, up, fpp, fpp, upp]
        lib.pt_simplify_opts_default.argtypes = [C.POINTER(SimplifyOpts)]
        lib.pt_mesh_simplify.argtypes = [C.c_void_p, C.POINTER(SimplifyOpts)] + simp_args
        lib.pt_mesh_simplify_host.argtypes = [C.POINTER(SimplifyOpts)] + simp_args
    if os.environ.get("PT_AMD_LIB") and not hasattr(lib, "pt_shard_range"):
        return lib                                   # A/B run against a build that predates the multi-GPU entry points
    lib.pt_shard_range.argtypes = [C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.pt_shard_range.restype = None
    lib.pt_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_double, C.POINTER(C.c_void_p)]
    lib.pt_comm_destroy.argtypes = [C.c_void_p]
    lib.pt_comm_destroy.restype = None
    lib.pt_comm_rank.argtypes = [C.c_void_p]
    lib.pt_comm_world.argtypes = [C.c_void_p]
    lib.pt_comm_barrier.argtypes = [C.c_void_p]
    lib.pt_comm_allreduce_f64.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
    lib.pt_bootstrap_exchange.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.c_double]
    lib.pt_render_multi.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.POINTER(RenderOpts), C.POINTER(RenderStats)]
    return lib


lib = _load()


SAMPLERS = {"independent": 0, "sobol": 1}   # pt_scene_set_sampler's kinds
LIGHT_SAMPLING = {"reference": 0, "exact": 1}   # pt_scene_set_light_sampling's kinds
PROJECTIONS = {"perspective": 0, "orthographic": 1, "fisheye": 2, "panorama": 3}   # pt_scene_set_projection's kinds


def _check(rc, what="pt call"):
    if rc < 0:
        raise PtError(f"{what}: {lib.pt_last_error().decode()}")
    return rc


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def decode_image_rgb8(path: str) -> np.ndarray:
    """JPEG/PNG -> RGB8 (H, W, 3) via PILLOW — an independent decoder, kept for the tests (the oracle is fed these pixels, the
    product decodes the same files itself: pt_load_jpeg_rgb8 / pt_load_png_rgb8) and for formats the library has no decoder
    for (hand the result to Scene.register_image). Alpha is dropped like ``to_rgb8`` does, texture.rs:67."""
    from PIL import Image

    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8))


class Context:
    """One GPU. Raises PtError when no HIP device is present (no CPU fallback)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        _check(lib.pt_ctx_create(device, C.byref(h)), "pt_ctx_create")
        self.handle = h

    def name(self) -> str:
        buf = C.create_string_buffer(256)
        _check(lib.pt_device_name(self.handle, buf, 256))
        return buf.value.decode()

    def close(self):
        if self.handle:
            lib.pt_ctx_destroy(self.handle)
            self.handle = None

    def math_probe(self, which: int, ab: np.ndarray) -> np.ndarray:
        ab = np.ascontiguousarray(ab, dtype=np.float64).reshape(-1, 2)
        out = np.empty(len(ab), dtype=np.float64)
        _check(lib.pt_math_probe(self.handle, which, ab.ctypes.data, len(ab), out.ctypes.data), "pt_math_probe")
        return out

    def sampler_probe(self, kind, seed: int, pixel: int, sample_begin: int, n_samples: int, draw_begin: int, n_draws: int) -> np.ndarray:
        """The 64-bit values of single draws [draw_begin, +n_draws) of samples [sample_begin, +n_samples) of a pixel, by the
        device functions the kernels call; uint64 array of shape (n_samples, n_draws)."""
        out = np.empty((n_samples, n_draws), dtype=np.uint64)
        _check(lib.pt_sampler_probe(self.handle, SAMPLERS.get(kind, kind), seed, pixel, sample_begin, n_samples, draw_begin, n_draws, out.ctypes.data),
               "pt_sampler_probe")
        return out

    def resolve_u8(self, accum: np.ndarray, total_spp: int) -> np.ndarray:
        accum = np.ascontiguousarray(accum, dtype=np.float64)
        out = np.empty(accum.shape, dtype=np.uint8)
        _check(lib.pt_resolve_u8(self.handle, accum.ctypes.data, accum.size // 3, total_spp, out.ctypes.data), "pt_resolve_u8")
        return out

    def resolve_u8_counts(self, accum: np.ndarray, spp_per_pixel: np.ndarray) -> np.ndarray:
        """resolve_u8 with each pixel's own sample count (the counts of Scene.render_adaptive)."""
        accum = np.ascontiguousarray(accum, dtype=np.float64)
        counts = np.ascontiguousarray(spp_per_pixel, dtype=np.uint32)
        assert counts.size * 3 == accum.size
        out = np.empty(accum.shape, dtype=np.uint8)
        _check(lib.pt_resolve_u8_counts(self.handle, accum.ctypes.data, counts.size, counts.ctypes.data, out.ctypes.data), "pt_resolve_u8_counts")
        return out

    def denoise(self, sum_a: np.ndarray, n_a: int, sum_b: np.ndarray, n_b: int, aov: np.ndarray, n_aov: int, iterations: int = 5,
                sigma_l: float = 4.0, sigma_z: float = 0.1) -> np.ndarray:
        """pt_denoise: the (H, W, 3) denoised MEANS of a frame rendered as two disjoint sample sets (sums `sum_a` of n_a samples,
        `sum_b` of n_b), guided by the (H, W, 8) first-hit sums `aov` of n_aov samples (Scene.render_aovs)."""
        sum_a = np.ascontiguousarray(sum_a, dtype=np.float64)
        sum_b = np.ascontiguousarray(sum_b, dtype=np.float64)
        aov = np.ascontiguousarray(aov, dtype=np.float64)
        h, w = sum_a.shape[0], sum_a.shape[1]
        assert sum_a.shape == (h, w, 3) and sum_b.shape == (h, w, 3) and aov.shape == (h, w, 8)
        out = np.empty((h, w, 3), dtype=np.float64)
        opts = DenoiseOpts(iterations, sigma_l, sigma_z)
        _check(lib.pt_denoise(self.handle, w, h, sum_a.ctypes.data, n_a, sum_b.ctypes.data, n_b, aov.ctypes.data, n_aov, C.byref(opts),
                              out.ctypes.data), "pt_denoise")
        return out

    def film(self, sums, total_spp: Optional[int] = None, counts=None, *, device_ptrs=None, **opts):
        """pt_film_develop: (hdr, rgb8) of a frame of sample SUMS: hdr the scene-linear (H, W, 3) f64 image after exposure and glare,
        rgb8 the (H, W, 3) bytes after the tone curve. `sums`: (H, W, 3) sums of `total_spp` samples, or with `counts` (H, W) of each
        pixel's own count. `opts`: the fields of FilmOpts (tonemap by name or number); none = pt_resolve_u8's bytes.
        device_ptrs = (width, height, sums, counts or None, hdr or None, rgb8 or None) as device addresses (e.g. tensor.data_ptr())
        runs on device buffers instead (on_device): `sums` is then ignored and None is returned."""
        o = FilmOpts(**opts)
        if device_ptrs is not None:
            w, h, d_sums, d_counts, d_hdr, d_rgb = device_ptrs
            o.on_device = 1
            _check(lib.pt_film_develop(self.handle, w, h, d_sums, total_spp or 0, d_counts, C.byref(o), d_hdr, d_rgb), "pt_film_develop")
            return None
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        h, w = sums.shape[0], sums.shape[1]
        assert sums.shape == (h, w, 3)
        cnt = None
        if counts is not None:
            cnt = np.ascontiguousarray(counts, dtype=np.uint32)
            assert cnt.size == h * w
        o.on_device = 0
        hdr = np.empty((h, w, 3), dtype=np.float64)
        rgb8 = np.empty((h, w, 3), dtype=np.uint8)
        _check(lib.pt_film_develop(self.handle, w, h, sums.ctypes.data, total_spp or 0, cnt.ctypes.data if cnt is not None else None, C.byref(o),
                                   hdr.ctypes.data, rgb8.ctypes.data), "pt_film_develop")
        return hdr, rgb8

    def sky_bake(self, w: int, h: int, *, device_ptr=None, **opts):
        """pt_sky_bake: the physical sky as an (h, w, 3) float32 lat-long map, disc included. `opts`: the fields of SkyOpts.
        device_ptr: the address of w*h*3 floats of device memory to fill instead (e.g. tensor.data_ptr()); None is returned then."""
        o = SkyOpts(**opts)
        if device_ptr is not None:
            _check(lib.pt_sky_bake(self.handle, C.byref(o), w, h, device_ptr, 1), "pt_sky_bake")
            return None
        out = np.empty((h, w, 3), dtype=np.float32)
        _check(lib.pt_sky_bake(self.handle, C.byref(o), w, h, out.ctypes.data, 0), "pt_sky_bake")
        return out

    def tessellate(self, pos, idx, nrm=None, uv=None, levels=1, height=None, scale=1.0, midlevel=0.5, wrap="clamp", normals="auto"):
        """pt_mesh_tessellate: `levels` 1-to-4 subdivisions of a triangle mesh on the GPU, then displacement along the normals by the
        (H, W) float32 image `height` (scale * (h - midlevel)) -> (pos, idx, nrm | None, uv | None), ready for Scene.mesh.
        wrap: "clamp" / "repeat"; normals: "auto" / "keep" / "smooth" / "none" (include/pt_amd.h has the rule)."""
        return _tessellate(self.handle, pos, idx, nrm, uv, TessOpts(levels, height, scale, midlevel, wrap, normals))

    def subdivide(self, pos, idx, uv=None, crease=None, levels=1, crease_deg=None, corner_deg=None, limit=False, normals="smooth"):
        """pt_mesh_subdivide: `levels` levels of Loop subdivision of a triangle mesh on the GPU -> (pos, idx, nrm | None, uv | None, crease),
        ready for Scene.mesh or Context.tessellate. crease: one flag per index, crease[3f + k] marks edge k of face f as sharp; crease_deg:
        the angle between two faces' normals above which their edge is sharp; corner_deg: the angle between a crease vertex's two sharp edges
        below which it is a corner; limit: push the vertices to the limit surface; normals: "smooth" / "none" (include/pt_amd.h has the rule)."""
        return _subdivide(self.handle, pos, idx, uv, crease, SubdivOpts(levels, _cos_deg(crease_deg, -2.0), _cos_deg(corner_deg, 2.0), limit, normals))

    def isosurface(self, values, box_lo, box_hi, iso=0.5, closed=False, outside=0.0, normals="gradient"):
        """pt_mesh_isosurface: the level set `iso` of a (nz, ny, nx) float32 grid (pt_mat_medium_grid's layout: the samples sit at the
        cell centres of the box) as a triangle mesh, by marching tetrahedra on the GPU -> (pos, idx, nrm | None), ready for Scene.mesh,
        Context.subdivide or Context.tessellate. closed: a layer of `outside` samples around the grid closes the surface; normals:
        "gradient" / "smooth" / "none" (include/pt_amd.h has the rule)."""
        return _isosurface(self.handle, values, box_lo, box_hi, IsoOpts(iso, closed, outside, normals))

    def mesh_sdf(self, pos, idx, dims, box_lo, box_hi, what="depth", fill="nonzero", negate=False, band=0.0, ramp=None):
        """pt_mesh_sdf: a triangle mesh sampled at the cell centres of an (nx, ny, nz) = dims grid over the box, on the GPU -> a (nz, ny, nx)
        float32 array in Scene.mat_medium_grid's and Context.isosurface's layout. what: "depth" (signed distance, positive inside) /
        "distance" (unsigned, open meshes welcome) / "occupancy" / "density" (min(d, ramp) / ramp inside, 0 outside); fill: "nonzero" /
        "odd"; band > 0 caps the distances (include/pt_amd.h has the rule)."""
        return _mesh_sdf(self.handle, pos, idx, dims, box_lo, box_hi, SdfOpts(what, fill, negate, band, ramp))

    def simplify(self, pos, idx, uv=None, mode="cluster", cell=0.0, grid_n=64, placement="quadric", reg=1e-3, dedup=True, normals="smooth"):
        """pt_mesh_simplify: a triangle mesh welded (mode "weld": vertices of equal position become one) or simplified (mode "cluster":
        the vertices of each cubic cell become one, placed by the cell's quadric or at their mean) on the GPU -> (pos, idx, nrm | None,
        uv | None, map), ready for Scene.mesh, Context.subdivide, Context.tessellate or Context.mesh_sdf. cell: the cells' edge, or 0:
        the longest extent / grid_n; dedup: coincident triangles cancel by orientation; map[v]: the output vertex of input vertex v or
        0xFFFFFFFF (include/pt_amd.h has the rule)."""
        return _simplify(self.handle, pos, idx, uv, SimplifyOpts(mode, cell, grid_n, placement, reg, dedup, normals))

    def sky_probe(self, dirs: np.ndarray, **opts) -> np.ndarray:
        """pt_sky_probe: sky_eval by the bake kernel's device function: (n, 3) unit directions -> (n, 3) radiance, no disc."""
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        out = np.empty((len(dirs), 3), dtype=np.float64)
        o = SkyOpts(**opts)
        _check(lib.pt_sky_probe(self.handle, C.byref(o), dirs.ctypes.data, len(dirs), out.ctypes.data), "pt_sky_probe")
        return out


class _MeshOut:
    """The six outputs of pt_mesh_tessellate / pt_mesh_grid: handed to the call by reference, copied into arrays, freed with pt_free."""

    def __init__(self):
        self.pos, self.idx, self.nrm, self.uv = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
        self.n_pos, self.n_idx = C.c_uint32(), C.c_uint32()

    def refs(self):
        return (C.byref(self.pos), C.byref(self.n_pos), C.byref(self.idx), C.byref(self.n_idx), C.byref(self.nrm), C.byref(self.uv))

    def take(self):
        n, m = self.n_pos.value, self.n_idx.value
        arr = lambda p, k, dt: np.ctypeslib.as_array(p, (n * k,)).copy().reshape(-1, k) if n else np.zeros((0, k), dt)
        out = (arr(self.pos, 3, np.float32), np.ctypeslib.as_array(self.idx, (m,)).copy() if m else np.zeros(0, np.uint32),
               arr(self.nrm, 3, np.float32) if self.nrm else None, arr(self.uv, 2, np.float32) if self.uv else None)
        self.free()
        return out

    def free(self):
        for p in (self.pos, self.idx, self.nrm, self.uv):
            if p:
                lib.pt_free(p)


def _mesh_in(pos, idx, nrm, uv):
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
    nrm = None if nrm is None else np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 3)
    uv = None if uv is None else np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    args = (len(pos), pos.ctypes.data, len(idx), idx.ctypes.data, 0 if nrm is None else len(nrm), None if nrm is None else nrm.ctypes.data,
            0 if uv is None else len(uv), None if uv is None else uv.ctypes.data)
    return args, (pos, idx, nrm, uv)   # (the arrays: kept alive by the caller for the length of the call)


def _tessellate(ctx, pos, idx, nrm, uv, opts):
    args, keep = _mesh_in(pos, idx, nrm, uv)
    out = _MeshOut()
    if ctx is None:
        rc = lib.pt_mesh_tessellate_host(C.byref(opts), *args, *out.refs())
    else:
        rc = lib.pt_mesh_tessellate(ctx, C.byref(opts), *args, *out.refs())
    if rc < 0:
        out.free()
    _check(rc, "pt_mesh_tessellate_host" if ctx is None else "pt_mesh_tessellate")
    return out.take()


def tessellate_host(pos, idx, nrm=None, uv=None, levels=1, height=None, scale=1.0, midlevel=0.5, wrap="clamp", normals="auto"):
    """pt_mesh_tessellate_host: Context.tessellate on the host, the same bytes (no context needed)."""
    return _tessellate(None, pos, idx, nrm, uv, TessOpts(levels, height, scale, midlevel, wrap, normals))


def _subdivide(ctx, pos, idx, uv, crease, opts):
    args, keep = _mesh_in(pos, idx, None, uv)
    args = args[:4] + args[6:]                       # (no normals go in)
    if crease is not None:
        crease = np.ascontiguousarray(crease, dtype=np.uint8).reshape(-1)
        if len(crease) != args[2]:
            raise ValueError("crease must hold one flag per index")
    out, flags = _MeshOut(), C.POINTER(C.c_uint8)()
    tail = (None if crease is None else crease.ctypes.data, *out.refs(), C.byref(flags))
    if ctx is None:
        rc = lib.pt_mesh_subdivide_host(C.byref(opts), *args, *tail)
    else:
        rc = lib.pt_mesh_subdivide(ctx, C.byref(opts), *args, *tail)
    name = "pt_mesh_subdivide_host" if ctx is None else "pt_mesh_subdivide"
    if rc < 0:
        out.free()
        if flags:
            lib.pt_free(flags)
    _check(rc, name)
    m = out.n_idx.value
    cr = np.ctypeslib.as_array(flags, (m,)).copy() if m else np.zeros(0, np.uint8)
    lib.pt_free(flags)
    return (*out.take(), cr)


def subdivide_host(pos, idx, uv=None, crease=None, levels=1, crease_deg=None, corner_deg=None, limit=False, normals="smooth"):
    """pt_mesh_subdivide_host: Context.subdivide on the host, the same bytes (no context needed)."""
    return _subdivide(None, pos, idx, uv, crease, SubdivOpts(levels, _cos_deg(crease_deg, -2.0), _cos_deg(corner_deg, 2.0), limit, normals))


def _isosurface(ctx, values, box_lo, box_hi, opts):
    values = np.ascontiguousarray(values, dtype=np.float32)
    if values.ndim != 3:
        raise ValueError("values must be a (nz, ny, nx) grid")
    nz, ny, nx = values.shape
    lo, hi = np.ascontiguousarray(box_lo, dtype=np.float64).reshape(3), np.ascontiguousarray(box_hi, dtype=np.float64).reshape(3)
    out = _MeshOut()
    refs = out.refs()[:5]                            # (no texcoords come out)
    args = (nx, ny, nz, values.ctypes.data, lo.ctypes.data, hi.ctypes.data)
    if ctx is None:
        rc = lib.pt_mesh_isosurface_host(C.byref(opts), *args, *refs)
    else:
        rc = lib.pt_mesh_isosurface(ctx, C.byref(opts), *args, *refs)
    if rc < 0:
        out.free()
    _check(rc, "pt_mesh_isosurface_host" if ctx is None else "pt_mesh_isosurface")
    return out.take()[:3]


def isosurface_host(values, box_lo, box_hi, iso=0.5, closed=False, outside=0.0, normals="gradient"):
    """pt_mesh_isosurface_host: Context.isosurface on the host, the same bytes (no context needed)."""
    return _isosurface(None, values, box_lo, box_hi, IsoOpts(iso, closed, outside, normals))


def _simplify(ctx, pos, idx, uv, opts):
    args, keep = _mesh_in(pos, idx, None, uv)
    args = args[:4] + args[6:]                       # (no normals go in)
    out, vmap = _MeshOut(), C.POINTER(C.c_uint32)()
    if ctx is None:
        rc = lib.pt_mesh_simplify_host(C.byref(opts), *args, *out.refs(), C.byref(vmap))
    else:
        rc = lib.pt_mesh_simplify(ctx, C.byref(opts), *args, *out.refs(), C.byref(vmap))
    if rc < 0:
        out.free()
        if vmap:
            lib.pt_free(vmap)
    _check(rc, "pt_mesh_simplify_host" if ctx is None else "pt_mesh_simplify")
    n = args[0]
    vm = np.ctypeslib.as_array(vmap, (n,)).copy() if n else np.zeros(0, np.uint32)
    lib.pt_free(vmap)
    return (*out.take(), vm)


def simplify_host(pos, idx, uv=None, mode="cluster", cell=0.0, grid_n=64, placement="quadric", reg=1e-3, dedup=True, normals="smooth"):
    """pt_mesh_simplify_host: Context.simplify on the host, the same bytes (no context needed)."""
    return _simplify(None, pos, idx, uv, SimplifyOpts(mode, cell, grid_n, placement, reg, dedup, normals))


def _mesh_sdf(ctx, pos, idx, dims, box_lo, box_hi, opts):
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
    nx, ny, nz = (int(n) for n in dims)
    if min(nx, ny, nz) < 0 or max(nx, ny, nz) >= 2**32:
        raise ValueError("dims must be three 32-bit unsigned integers")
    lo, hi = np.ascontiguousarray(box_lo, dtype=np.float64).reshape(3), np.ascontiguousarray(box_hi, dtype=np.float64).reshape(3)
    big = nx * ny * nz > 2**28 or min(nx, ny, nz) < 2                       # (refused by the library: no array of that size is made first)
    out = np.zeros(1 if big else (nz, ny, nx), dtype=np.float32)
    args = (len(pos), pos.ctypes.data, len(idx), idx.ctypes.data, nx, ny, nz, lo.ctypes.data, hi.ctypes.data, out.ctypes.data)
    if ctx is None:
        rc = lib.pt_mesh_sdf_host(C.byref(opts), *args)
    else:
        rc = lib.pt_mesh_sdf(ctx, C.byref(opts), *args)
    _check(rc, "pt_mesh_sdf_host" if ctx is None else "pt_mesh_sdf")
    return out


def mesh_sdf_host(pos, idx, dims, box_lo, box_hi, what="depth", fill="nonzero", negate=False, band=0.0, ramp=None):
    """pt_mesh_sdf_host: Context.mesh_sdf on the host, the same bytes (no context needed)."""
    return _mesh_sdf(None, pos, idx, dims, box_lo, box_hi, SdfOpts(what, fill, negate, band, ramp))


def mesh_fit_grid(pos, n_longest: int, margin_cells: float = 2.0):
    """pt_mesh_fit_grid: cubic cells around a mesh, n_longest of them along its longest extent, margin_cells of them free on either side
    -> ((nx, ny, nz), box_lo, box_hi) for mesh_sdf."""
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    dims, lo, hi = np.zeros(3, np.uint32), np.zeros(3, np.float64), np.zeros(3, np.float64)
    _check(lib.pt_mesh_fit_grid(len(pos), pos.ctypes.data, int(n_longest), float(margin_cells), dims.ctypes.data, lo.ctypes.data, hi.ctypes.data), "pt_mesh_fit_grid")
    return (int(dims[0]), int(dims[1]), int(dims[2])), lo, hi


def mesh_grid(q, u, v, nu: int, nv: int):
    """pt_mesh_grid: the (nu x nv)-cell triangle mesh that stands in for pt_quad(q, u, v) -> (pos, idx, nrm, uv)."""
    out = _MeshOut()
    rc = lib.pt_mesh_grid(_d3(q), _d3(u), _d3(v), nu, nv, *out.refs())
    if rc < 0:
        out.free()
    _check(rc, "pt_mesh_grid")
    return out.take()


def height_from_rgb8(rgb8: np.ndarray) -> np.ndarray:
    """pt_height_from_rgb8: (H, W, 3) uint8 -> (H, W) float32 Rec. 709 luminance in [0, 1]: a height image for tessellate."""
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w = rgb8.shape[:2]
    out = np.empty((h, w), np.float32)
    _check(lib.pt_height_from_rgb8(w, h, rgb8.ctypes.data, out.ctypes.data), "pt_height_from_rgb8")
    return out


def sky_eval(dirs: np.ndarray, **opts) -> np.ndarray:
    """pt_sky_eval (host only): (n, 3) unit directions -> (n, 3) radiance of the physical sky: the sky above, the ground below, no disc."""
    dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    out = np.empty((len(dirs), 3), dtype=np.float64)
    o = SkyOpts(**opts)
    _check(lib.pt_sky_eval(C.byref(o), dirs.ctypes.data, len(dirs), out.ctypes.data), "pt_sky_eval")
    return out


def sky_sun_irradiance(**opts) -> np.ndarray:
    """pt_sky_sun_irradiance (host only): the irradiance (rgb) the sun of these options brings to a surface facing it: what the baked disc
    carries, and what Scene.light_directional needs to stand in for it. Zeros when the sun is not above the horizon."""
    out = (C.c_double * 3)()
    o = SkyOpts(**opts)
    _check(lib.pt_sky_sun_irradiance(C.byref(o), out), "pt_sky_sun_irradiance")
    return np.array(out[:], dtype=np.float64)


def adaptive_schedule(min_spp: int, max_spp: int):
    """Round boundaries [0, b_1, ..., max_spp] of Scene.render_adaptive (pt_adaptive_schedule)."""
    n = _check(lib.pt_adaptive_schedule(min_spp, max_spp, None, 0), "pt_adaptive_schedule")
    b = np.zeros(n, dtype=np.uint32)
    _check(lib.pt_adaptive_schedule(min_spp, max_spp, b.ctypes.data, n), "pt_adaptive_schedule")
    return [int(x) for x in b]


def shard_range(spp: int, rank: int, world: int):
    """Sample range [lo, hi) that rank `rank` of `world` renders (pt_shard_range)."""
    lo, hi = C.c_uint32(), C.c_uint32()
    lib.pt_shard_range(spp, rank, world, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def bootstrap_exchange(path: str, rank: int, payload: bytes, timeout_s: float = 60.0) -> bytes:
    """The file rendezvous pt_comm_create uses for the RCCL unique id: rank 0 publishes `payload`, the others get it."""
    buf = C.create_string_buffer(payload, len(payload))
    _check(lib.pt_bootstrap_exchange(path.encode(), rank, buf, len(payload), timeout_s), "pt_bootstrap_exchange")
    return buf.raw


class Comm:
    """One rank of an RCCL communicator over the GPUs of a node (one process per GPU)."""

    def __init__(self, ctx: Context, rank: int, world: int, id_path: Optional[str] = None, timeout_s: float = 120.0):
        h = C.c_void_p()
        _check(lib.pt_comm_create(ctx.handle, rank, world, None if id_path is None else id_path.encode(), timeout_s, C.byref(h)), "pt_comm_create")
        self.handle, self.ctx = h, ctx
        self.rank, self.world = int(lib.pt_comm_rank(h)), int(lib.pt_comm_world(h))     # what the communicator says, not what was asked for

    def close(self):
        if self.handle:
            lib.pt_comm_destroy(self.handle)
            self.handle = None

    def barrier(self):
        _check(lib.pt_comm_barrier(self.handle), "pt_comm_barrier")

    def allreduce(self, values, op: str = "sum") -> np.ndarray:
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        _check(lib.pt_comm_allreduce_f64(self.handle, v.ctypes.data, v.size, 1 if op == "max" else 0), "pt_comm_allreduce_f64")
        return v


class Scene:
    """World + builder (hittable/world.rs). Method names follow the C ABI minus the prefix."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.handle = C.c_void_p(lib.pt_scene_create(ctx.handle))
        if not self.handle:
            raise PtError("pt_scene_create failed")

    def close(self):
        if self.handle:
            lib.pt_scene_destroy(self.handle)
            self.handle = None

    # generic dispatcher used by tests that replay one scene description onto this API and
    # onto the oracle's isomorphic one
    def call(self, name: str, *args):
        return getattr(self, name)(*args)

    def tex_solid_rgb(self, r, g, b): return _check(lib.pt_tex_solid_rgb(self.handle, r, g, b), "tex_solid_rgb")
    def tex_solid_f(self, v): return _check(lib.pt_tex_solid_f(self.handle, v), "tex_solid_f")
    def tex_checker(self, scale, t1, t2): return _check(lib.pt_tex_checker(self.handle, scale, t1, t2), "tex_checker")

    def tex_image_rgb8(self, img: np.ndarray):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w = img.shape[:2]
        return _check(lib.pt_tex_image_rgb8(self.handle, w, h, img.ctypes.data), "tex_image_rgb8")

    def tex_image_rgbf32(self, img: np.ndarray):
        """ImageTexture that keeps f32 samples (no to_rgb8 squash, texture.rs:67): the float-HDR option."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        h, w = img.shape[:2]
        return _check(lib.pt_tex_image_rgbf32(self.handle, w, h, img.ctypes.data), "tex_image_rgbf32")

    def tex_sky(self, w: int, h: int, **opts):
        """pt_tex_sky: the physical sky (the fields of SkyOpts) baked on the GPU into a w x h float image texture: use the handle as
        Camera.env_tex with env_is_map = 1."""
        o = SkyOpts(**opts)
        return _check(lib.pt_tex_sky(self.handle, C.byref(o), w, h), "pt_tex_sky")

    def set_float_hdr(self, on: bool = True):
        """Scene scripts (build_scene) load Radiance .hdr files as f32 textures from now on."""
        return _check(lib.pt_scene_set_float_hdr(self.handle, 1 if on else 0), "set_float_hdr")

    def set_env_sampling(self, f: float):
        """Environment importance sampling with mixture weight f, 0 <= f < 1 (0 = off, the default)."""
        return _check(lib.pt_scene_set_env_sampling(self.handle, float(f)), "set_env_sampling")

    def env_sampling(self) -> float:
        return lib.pt_scene_env_sampling(self.handle)

    def set_sampler(self, kind):
        """Where the paths' random numbers come from: "independent" (0, the default: the reference's draws) or "sobol" (1: an
        Owen-scrambled Sobol sequence per pixel; the rule is in include/pt_amd.h)."""
        kind = SAMPLERS.get(kind, kind)
        if isinstance(kind, bool) or not isinstance(kind, int):
            raise PtError(f"set_sampler: unknown sampler {kind!r}")
        return _check(lib.pt_scene_set_sampler(self.handle, kind), "set_sampler")

    def sampler(self) -> int:
        return lib.pt_scene_sampler(self.handle)

    def set_light_sampling(self, kind):
        """How mesh and sphere lights are sampled: "reference" (0, the default: the reference's lights.sample / lights.pdf) or "exact"
        (1: area-weighted mesh lights whose pdf walks the mesh's BVH, cone-sampled sphere lights; the rule is in include/pt_amd.h,
        DESIGN.md §15). Needs no world_build."""
        kind = LIGHT_SAMPLING.get(kind, kind)
        if isinstance(kind, bool) or not isinstance(kind, int):
            raise PtError(f"set_light_sampling: unknown kind {kind!r}")
        return _check(lib.pt_scene_set_light_sampling(self.handle, kind), "set_light_sampling")

    def light_sampling(self) -> int:
        return lib.pt_scene_light_sampling(self.handle)

    def light_probe(self, which: int, arr: np.ndarray) -> np.ndarray:
        """lights.sample / lights.pdf as the kernels call them, of the current light-sampling kind. which 0: arr = (n, 4) (origin.xyz,
        time) -> (n, 6) {dir.xyz, light index, face index or -1, draws consumed}, row i with the independent sampler's draws of (seed 0,
        pixel i, sample 0) from draw 0; which 1: arr = (n, 7) (origin.xyz, direction.xyz, time) -> (n,) lights.pdf values."""
        if which not in (0, 1):
            raise PtError("light_probe: which must be 0 or 1")
        arr = np.ascontiguousarray(arr, dtype=np.float64).reshape((-1, 4 if which == 0 else 7))
        out = np.empty((len(arr), 6) if which == 0 else (len(arr),), dtype=np.float64)
        _check(lib.pt_light_probe(self.handle, which, arr.ctypes.data, len(arr), out.ctypes.data), "pt_light_probe")
        return out

    # ---- punctual lights (the rule is in include/pt_amd.h). The list takes effect at the next world_build. ----
    def light_point(self, position, power):
        """A point light of the given power in W per channel (pt_light_point: PointLight::new of the reference); returns its index."""
        return _check(lib.pt_light_point(self.handle, _d3(position), _d3(power)), "light_point")

    def light_spot(self, position, target, inner_deg, outer_deg, intensity):
        """A spot light aimed at `target`: full intensity (W/sr) inside the inner cone, a smoothstep to zero at the outer one; angles from the axis."""
        return _check(lib.pt_light_spot(self.handle, _d3(position), _d3(target), float(inner_deg), float(outer_deg), _d3(intensity)), "light_spot")

    def light_directional(self, direction, irradiance):
        """A sun: light travelling along `direction`, `irradiance` on a plane facing it (pt_light_directional)."""
        return _check(lib.pt_light_directional(self.handle, _d3(direction), _d3(irradiance)), "light_directional")

    def clear_punctual_lights(self): return _check(lib.pt_scene_clear_punctual_lights(self.handle), "clear_punctual_lights")
    def punctual_count(self) -> int: return _check(lib.pt_scene_punctual_count(self.handle), "pt_scene_punctual_count")

    def punctual_light(self, k) -> np.ndarray:
        """Light k's record exactly as stored, 16 doubles: kind, pos.xyz, axis.xyz, I.rgb, cos_i, cos_o, four zeros."""
        out = (C.c_double * 16)()
        _check(lib.pt_scene_punctual_light(self.handle, int(k), out), "pt_scene_punctual_light")
        return np.array(out[:], dtype=np.float64)

    def set_punctual_fraction(self, f):
        """The selector's share of the punctual branch at a bounce, 0 < f < 1 (default 0.5)."""
        return _check(lib.pt_scene_set_punctual_fraction(self.handle, float(f)), "set_punctual_fraction")

    def punctual_fraction(self) -> float: return lib.pt_scene_punctual_fraction(self.handle)

    def set_punctual_media(self, on):
        """Light shafts: 1 lets the punctual lights light participating media (homogeneous and grid media), 0 (default) refuses the pair."""
        return _check(lib.pt_scene_set_punctual_media(self.handle, int(on)), "set_punctual_media")

    def punctual_media(self) -> int: return lib.pt_scene_punctual_media(self.handle)

    def set_punctual_selection(self, kind):
        """How the punctual branch picks its light: "uniform" (0, the default) or "grid" (1: by importance per scene cell, the light grid of
        DESIGN.md §26). Takes effect at the next world_build."""
        kind = {"uniform": 0, "grid": 1}.get(kind, kind)
        if not isinstance(kind, (int, np.integer)) or isinstance(kind, bool):
            raise PtError('set_punctual_selection: the kind is "uniform" or "grid"')
        return _check(lib.pt_scene_set_punctual_selection(self.handle, int(kind)), "set_punctual_selection")

    def punctual_selection(self) -> str: return ("uniform", "grid")[_check(lib.pt_scene_punctual_selection(self.handle), "pt_scene_punctual_selection")]

    def set_punctual_grid(self, nx=0, ny=0, nz=0, box=None):
        """The light grid's dims (0, 0, 0: automatic; else each in 1..64) and box (lo.xyz, hi.xyz; None: the world's bounds at the build).
        Takes effect at the next world_build."""
        if min(int(nx), int(ny), int(nz)) < 0:
            raise PtError("set_punctual_grid: the dims are 0, 0, 0 (automatic) or each in 1..64")
        b = None if box is None else np.ascontiguousarray(box, dtype=np.float64).reshape(6)
        return _check(lib.pt_scene_set_punctual_grid(self.handle, int(nx), int(ny), int(nz), None if b is None else b.ctypes.data), "set_punctual_grid")

    def punctual_grid(self):
        """((nx, ny, nz), box6) of the light grid the last world_build used; raises when the grid is not in effect."""
        dims, box = np.zeros(3, dtype=np.uint32), np.zeros(6, dtype=np.float64)
        _check(lib.pt_scene_punctual_grid(self.handle, dims.ctypes.data, box.ctypes.data), "pt_scene_punctual_grid")
        return tuple(int(d) for d in dims), box

    def punctual_probe(self, which: int, arr: np.ndarray) -> np.ndarray:
        """The punctual branch's device functions as the kernels call them. which 0: arr = (n, 3) points -> (n, 9) {k, w.xyz, D, E.rgb, draws
        consumed}, row i with the independent sampler's draws of (seed 0, pixel i, sample 0) from draw 0; which 1: arr = (n, 4) (k, point.xyz)
        -> (n, 7) {w.xyz, D, E.rgb}. With the light grid in effect: which 2: arr = (n, 3) points -> (n, 11) {cell, k, p, draws consumed, w.xyz,
        D, E.rgb}; which 3: arr = (n, 2) (cell, k) -> (n,) C[cell][k]."""
        if which not in (0, 1, 2, 3):
            raise PtError("punctual_probe: which must be 0, 1, 2 or 3")
        arr = np.ascontiguousarray(arr, dtype=np.float64).reshape((-1, (3, 4, 3, 2)[which]))
        out = np.empty((len(arr), (9, 7, 11, 1)[which]), dtype=np.float64)
        if which == 3:
            out = out.reshape(-1)
        _check(lib.pt_punctual_probe(self.handle, which, arr.ctypes.data, len(arr), out.ctypes.data), "pt_punctual_probe")
        return out

    def set_projection(self, kind):
        """How a pixel becomes a camera ray: "perspective" (0, the default: the reference's pinhole / thin-lens camera), "orthographic"
        (1: parallel rays framing the perspective camera's focal plane), "fisheye" (2: equidistant, vfov across the image height) or
        "panorama" (3: an equirectangular image of everything around look_from, usable as an environment map; the rule is in
        include/pt_amd.h). Needs no world_build."""
        kind = PROJECTIONS.get(kind, kind)
        if isinstance(kind, bool) or not isinstance(kind, int):
            raise PtError(f"set_projection: unknown projection {kind!r}")
        return _check(lib.pt_scene_set_projection(self.handle, kind), "set_projection")

    def projection(self) -> int:
        return lib.pt_scene_projection(self.handle)

    def camera_probe(self, cam: "Camera", seed: int, pixels_samples: np.ndarray) -> np.ndarray:
        """The camera rays the kernels generate, under the scene's projection and sampler: pixels_samples = (n, 2) (pixel, sample) ->
        (n, 8) {origin.xyz, direction.xyz, time, draws consumed} of the sample's stream of `seed`. The world need not be built."""
        arr = np.ascontiguousarray(pixels_samples, dtype=np.float64).reshape(-1, 2)
        out = np.empty((len(arr), 8), dtype=np.float64)
        _check(lib.pt_camera_probe(self.handle, C.byref(cam), int(seed), arr.ctypes.data, len(arr), out.ctypes.data), "pt_camera_probe")
        return out

    def mat_medium(self, density: float, albedo=(1.0, 1.0, 1.0), g: float = 0.0):
        """A homogeneous participating medium (fog, smoke) as a material: the object that carries it is the medium's invisible
        boundary. density = sigma_t > 0, albedo = sigma_s / sigma_t per channel in [0, 1], |g| < 1 the Henyey-Greenstein asymmetry
        (the rule is in include/pt_amd.h)."""
        return _check(lib.pt_mat_medium(self.handle, float(density), float(albedo[0]), float(albedo[1]), float(albedo[2]), float(g)), "mat_medium")

    def mat_medium_grid(self, scale: float, albedo, g: float, values: np.ndarray, box_lo, box_hi):
        """A participating medium whose density varies in space (a smoke plume, a cloud): sigma_t(x) = scale * V(x), V the trilinear
        interpolation of `values`, a float32 array of shape (nz, ny, nx) of samples at the cell centres of the world-space box
        [box_lo, box_hi] (copied); 0 outside the box. Used like a mat_medium handle: on a closed object, or as the camera medium
        (unbounded). Sampled by delta tracking (the rule is in include/pt_amd.h)."""
        values = np.asarray(values)
        if values.ndim != 3:
            raise PtError("mat_medium_grid: values must have shape (nz, ny, nx)")
        values = np.ascontiguousarray(values, dtype=np.float32)
        nz, ny, nx = values.shape
        lo, hi = (C.c_double * 3)(*[float(v) for v in box_lo]), (C.c_double * 3)(*[float(v) for v in box_hi])
        return _check(lib.pt_mat_medium_grid(self.handle, float(scale), float(albedo[0]), float(albedo[1]), float(albedo[2]), float(g), nx, ny, nz,
                                             values.ctypes.data, lo, hi), "mat_medium_grid")

    def mat_medium_tinted(self, density: float, albedo=(1.0, 1.0, 1.0), g: float = 0.0, absorption=(0.0, 0.0, 0.0)):
        """A homogeneous medium with an absorption coefficient per channel on top of its scattering (coloured glass, tea, wax):
        density >= 0 (0 = no scattering, pure Beer-Lambert absorption), albedo and g as mat_medium, absorption >= 0 per channel and
        density + max(absorption) > 0 (the rule is in include/pt_amd.h)."""
        a = (C.c_double * 3)(*[float(v) for v in absorption])
        return _check(lib.pt_mat_medium_tinted(self.handle, float(density), float(albedo[0]), float(albedo[1]), float(albedo[2]), float(g), a),
                      "mat_medium_tinted")

    def mat_glass_set_interior(self, glass_mat: int, medium_mat: int):
        """The medium that fills objects of glass material `glass_mat` (any medium handle; -1 detaches): a path enters it when it
        refracts in, keeps it under internal reflection and leaves it when it refracts out. Rebuild the world after."""
        return _check(lib.pt_mat_glass_set_interior(self.handle, int(glass_mat), int(medium_mat)), "mat_glass_set_interior")

    def mat_glass_interior(self, glass_mat: int) -> int:
        return lib.pt_mat_glass_interior(self.handle, int(glass_mat))

    def mat_glass_set_dispersion(self, glass_mat: int, abbe: float):
        """Spectral dispersion of glass material `glass_mat`: its ior is read as n_d (587.56 nm) and `abbe` is the Abbe number V_d of a
        two-term Cauchy law (crown glass about 60, flint 30; smaller = more colour; 0 = off, the default). Every path then carries one
        wavelength, drawn per (seed, pixel, sample) and stratified under the Sobol sampler (the rule is in include/pt_amd.h, DESIGN.md
        §16). Rebuild the world after."""
        return _check(lib.pt_mat_glass_set_dispersion(self.handle, int(glass_mat), float(abbe)), "mat_glass_set_dispersion")

    def mat_glass_dispersion(self, glass_mat: int) -> float:
        """The Abbe number set with mat_glass_set_dispersion, 0.0 when off, -1.0 for a handle that is not a glass."""
        return lib.pt_mat_glass_dispersion(self.handle, int(glass_mat))

    def dispersion_probe(self, glass_mat: int, which: int, arr: np.ndarray, seed: int = 0) -> np.ndarray:
        """The device functions of dispersion that the kernels call, for dispersive glass `glass_mat`, under the scene's sampler kind.
        which 0: arr = (n, 2) (pixel, sample) -> (n, 7) {u, lambda in nm, bin, W_r, W_g, W_b, n(lambda)} of a path of `seed`;
        which 1: arr = (n,) wavelengths in nm -> (n,) n(lambda). The world need not be built."""
        if which not in (0, 1):
            raise PtError("dispersion_probe: which must be 0 or 1")
        arr = np.ascontiguousarray(arr, dtype=np.float64).reshape((-1, 2) if which == 0 else (-1,))
        out = np.empty((len(arr), 7) if which == 0 else (len(arr),), dtype=np.float64)
        _check(lib.pt_dispersion_probe(self.handle, int(glass_mat), which, int(seed), arr.ctypes.data, len(arr), out.ctypes.data), "pt_dispersion_probe")
        return out

    def set_camera_medium(self, mat: int):
        """The medium camera rays start in (a mat_medium / mat_medium_tinted / mat_medium_grid handle; -1 = none, the default)."""
        return _check(lib.pt_scene_set_camera_medium(self.handle, int(mat)), "set_camera_medium")

    def camera_medium(self) -> int:
        return lib.pt_scene_camera_medium(self.handle)

    def medium_probe(self, mat: int, which: int, arr: np.ndarray) -> np.ndarray:
        """The device functions of medium `mat` that the kernels call. which 0: arr = (n, 5) (u1, u2, dir.xyz) -> (n, 4)
        {new_dir.xyz, ph}; which 1: arr = (n,) unit draws -> (n,) free-flight distances. A mat_medium_grid medium also has which 2:
        arr = (n, 3) points -> (n,) sigma_t, and which 3: arr = (n, 7) (o.xyz, dir.xyz, t) -> (n, 3) {collided 0/1, s or 0, draws
        consumed}, row i tracked with the independent sampler's draws of (seed 0, pixel i, sample 0) from draw 0. which 4: arr = (n,)
        segment lengths -> (n, 3) the factors exp(-(a_c * l)) the medium's absorption puts on a throughput (exactly 1 where a_c = 0)."""
        cols_in, cols_out = {0: (5, 4), 1: (None, None), 2: (3, None), 3: (7, 3), 4: (None, 3)}.get(which, (None, None))
        arr = np.ascontiguousarray(arr, dtype=np.float64).reshape((-1, cols_in) if cols_in else (-1,))
        out = np.empty((len(arr), cols_out) if cols_out else (len(arr),), dtype=np.float64)
        _check(lib.pt_medium_probe(self.handle, int(mat), which, arr.ctypes.data, len(arr), out.ctypes.data), "pt_medium_probe")
        return out

    def mat_diffuse(self, color_tex, normal_map_tex=-1): return _check(lib.pt_mat_diffuse(self.handle, color_tex, normal_map_tex), "mat_diffuse")
    def mat_metal(self, color_tex, rough_tex): return _check(lib.pt_mat_metal(self.handle, color_tex, rough_tex), "mat_metal")
    def mat_glass(self, color_tex, rough_tex, aniso, ior): return _check(lib.pt_mat_glass(self.handle, color_tex, rough_tex, aniso, ior), "mat_glass")

    def mat_principled(self, color_tex, params: Sequence[float]):
        assert len(params) == 11
        return _check(lib.pt_mat_principled(self.handle, color_tex, (C.c_double * 11)(*params)), "mat_principled")

    def mat_light(self, tex): return _check(lib.pt_mat_light(self.handle, tex), "mat_light")
    def mat_mix(self, t, m1, m2): return _check(lib.pt_mat_mix(self.handle, t, m1, m2), "mat_mix")
    def mat_sheen(self, rgb, sheen_tint): return _check(lib.pt_mat_sheen(self.handle, rgb[0], rgb[1], rgb[2], sheen_tint), "mat_sheen")
    def mat_clearcoat(self, gloss): return _check(lib.pt_mat_clearcoat(self.handle, gloss), "mat_clearcoat")
    def sphere(self, r, p1, p2, mat): return _check(lib.pt_sphere(self.handle, r, _d3(p1), _d3(p2), mat), "sphere")
    def quad(self, q, u, v, mat): return _check(lib.pt_quad(self.handle, _d3(q), _d3(u), _d3(v), mat), "quad")
    def cuboid(self, a, b, mat): return _check(lib.pt_cuboid(self.handle, _d3(a), _d3(b), mat), "cuboid")

    def mesh(self, scale, pos, idx, nrm, uv, mat):
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        nrm = None if nrm is None else np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 3)
        uv = None if uv is None else np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        return _check(lib.pt_mesh(self.handle, scale, len(pos), pos.ctypes.data, len(idx), idx.ctypes.data,
                                  0 if nrm is None else len(nrm), None if nrm is None else nrm.ctypes.data,
                                  0 if uv is None else len(uv), None if uv is None else uv.ctypes.data, mat), "mesh")

    def instance(self, obj, axis, angle, translation): return _check(lib.pt_instance(self.handle, obj, _d3(axis), angle, _d3(translation)), "instance")

    def instance_moving(self, obj, axis, angle0, angle1, tr0, tr1):
        """An instance whose pose is keyframed over the ray's time (pt_instance_moving): angle0 -> angle1 about `axis`, tr0 -> tr1."""
        return _check(lib.pt_instance_moving(self.handle, obj, _d3(axis), float(angle0), float(angle1), _d3(tr0), _d3(tr1)), "instance_moving")

    def set_shutter(self, open, close):
        """The camera shutter (pt_scene_set_shutter): 0 <= open <= close <= 1; a camera ray's time is open + (close - open) * u."""
        return _check(lib.pt_scene_set_shutter(self.handle, float(open), float(close)), "set_shutter")

    def shutter(self):
        out = (C.c_double * 2)()
        _check(lib.pt_scene_shutter(self.handle, out), "pt_scene_shutter")
        return (out[0], out[1])

    def motion(self):
        """True when motion is in effect for the built world (pt_scene_motion)."""
        return _check(lib.pt_scene_motion(self.handle), "pt_scene_motion") == 1

    def entry_box(self, entry):
        """The f64 world box (lo.xyz, hi.xyz) of world entry `entry` (pt_world_entry_box)."""
        out = (C.c_double * 6)()
        _check(lib.pt_world_entry_box(self.handle, int(entry), out), "pt_world_entry_box")
        return np.array(out[:], dtype=np.float64)
    def world_add_object(self, obj): return _check(lib.pt_world_add_object(self.handle, obj), "world_add_object")
    def world_add_light(self, obj): return _check(lib.pt_world_add_light(self.handle, obj), "world_add_light")
    def world_build(self): return _check(lib.pt_world_build(self.handle), "world_build")
    def prim_count(self) -> int: return lib.pt_world_prim_count(self.handle)

    def set_device_bvh_threshold(self, min_triangles: int):
        """Meshes with at least this many triangles get their BVH built on the GPU at the next world_build (0 = never)."""
        _check(lib.pt_world_set_device_bvh_threshold(self.handle, min_triangles), "pt_world_set_device_bvh_threshold")

    def device_bvh_info(self):
        n, d = C.c_uint32(), C.c_uint32()
        _check(lib.pt_world_device_bvh_info(self.handle, C.byref(n), C.byref(d)), "pt_world_device_bvh_info")
        return n.value, d.value

    def register_image(self, name: str, img: np.ndarray):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w = img.shape[:2]
        _check(lib.pt_register_image(self.handle, name.encode(), w, h, img.ctypes.data), "register_image")

    def build_scene(self, scene_id: int, width: int, spp: int, asset_dir: str = ASSET_DIR, scene_seed: int = 1) -> Camera:
        """Run the reference's scene script N (main.rs `-s N`). Every image the scripts open (.hdr, .png, .jpg) is decoded by the
        library itself (pt_load_hdr_rgb8 / pt_load_png_rgb8 / pt_load_jpeg_rgb8); pixels handed over with register_image first
        take precedence."""
        cam = Camera()
        _check(lib.pt_build_scene(self.handle, scene_id, width, spp, asset_dir.encode(), scene_seed, C.byref(cam)), "pt_build_scene")
        return cam

    def render(self, cam: Camera, seed: int, spp_begin: int, spp_end: int, accum=None, slots_per_pixel: int = 0,
               profile: bool = False, device_ptr: Optional[int] = None, stream: Optional[int] = None, overwrite: bool = False):
        """Camera::render (camera.rs:79) without gamma/quantise: returns (accum, stats) where
        accum[(y, x, c)] += sum over samples [spp_begin, spp_end) of trace(y, x) (``overwrite``: = instead of +=).
        ``device_ptr``: write into device memory instead (e.g. ``tensor.data_ptr()``)."""
        h = image_height(cam)
        opts = RenderOpts(slots_per_pixel, 1 if device_ptr is not None else 0, 1 if profile else 0, 1 if overwrite else 0, stream)
        stats = RenderStats()
        if device_ptr is not None:
            ptr = C.c_void_p(device_ptr)
        else:
            if accum is None:
                accum = np.zeros((h, cam.image_width, 3), dtype=np.float64)
            assert accum.dtype == np.float64 and accum.flags["C_CONTIGUOUS"] and accum.size == h * cam.image_width * 3
            ptr = C.c_void_p(accum.ctypes.data)
        _check(lib.pt_render(self.handle, C.byref(cam), seed, spp_begin, spp_end, ptr, C.byref(opts), C.byref(stats)), "pt_render")
        return accum, stats

    def render_pixels(self, cam: Camera, seed: int, pixels, spp_begin: int, spp_end: int, accum=None, slots_per_pixel: int = 0,
                      profile: bool = False, device_ptr: Optional[int] = None, stream: Optional[int] = None, overwrite: bool = False):
        """render() restricted to `pixels` (row-major y*W+x, strictly ascending): only their entries of the (H, W, 3) frame are
        added to (``overwrite``: stored); the others are left as they are. Returns (accum, stats)."""
        h = image_height(cam)
        px = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
        opts = RenderOpts(slots_per_pixel, 1 if device_ptr is not None else 0, 1 if profile else 0, 1 if overwrite else 0, stream)
        stats = RenderStats()
        if device_ptr is not None:
            ptr = C.c_void_p(device_ptr)
        else:
            if accum is None:
                accum = np.zeros((h, cam.image_width, 3), dtype=np.float64)
            assert accum.dtype == np.float64 and accum.flags["C_CONTIGUOUS"] and accum.size == h * cam.image_width * 3
            ptr = C.c_void_p(accum.ctypes.data)
        _check(lib.pt_render_pixels(self.handle, C.byref(cam), seed, px.ctypes.data, px.size, spp_begin, spp_end, ptr, C.byref(opts),
                                    C.byref(stats)), "pt_render_pixels")
        return accum, stats

    def render_adaptive(self, cam: Camera, seed: int, min_spp: int, max_spp: int, threshold: float, slots_per_pixel: int = 0,
                        profile: bool = False, stream: Optional[int] = None):
        """Render to a noise target (pt_render_adaptive): each pixel stops once its two-sample-set error estimate is below
        `threshold` (see include/pt_amd.h for the exact rule). Returns (accum (H, W, 3) sums, counts (H, W) samples per pixel,
        stats summed over the passes)."""
        h = image_height(cam)
        accum = np.zeros((h, cam.image_width, 3), dtype=np.float64)
        counts = np.zeros((h, cam.image_width), dtype=np.uint32)
        opts = AdaptiveOpts(min_spp, max_spp, threshold, slots_per_pixel, 1 if profile else 0, stream)
        stats = RenderStats()
        _check(lib.pt_render_adaptive(self.handle, C.byref(cam), seed, C.byref(opts), accum.ctypes.data, counts.ctypes.data, C.byref(stats)),
               "pt_render_adaptive")
        return accum, counts, stats

    def render_aovs(self, cam: Camera, seed: int, spp_begin: int, spp_end: int, aov=None, overwrite: bool = False,
                    device_ptr: Optional[int] = None, stream: Optional[int] = None):
        """pt_render_aovs: first-hit feature SUMS over samples [spp_begin, spp_end), the camera rays of render() for the same
        seed: (H, W, 8) = albedo rgb, shading normal xyz, depth, hits. Added to ``aov`` (``overwrite``: stored);
        ``device_ptr``: device memory instead (then returns None)."""
        h = image_height(cam)
        opts = RenderOpts(0, 1 if device_ptr is not None else 0, 0, 1 if overwrite else 0, stream)
        if device_ptr is not None:
            ptr = C.c_void_p(device_ptr)
        else:
            if aov is None:
                aov = np.zeros((h, cam.image_width, 8), dtype=np.float64)
            assert aov.dtype == np.float64 and aov.flags["C_CONTIGUOUS"] and aov.size == h * cam.image_width * 8
            ptr = C.c_void_p(aov.ctypes.data)
        _check(lib.pt_render_aovs(self.handle, C.byref(cam), seed, spp_begin, spp_end, ptr, C.byref(opts)), "pt_render_aovs")
        return aov

    def render_multi(self, cam: Camera, seed: int, spp_total: int, comm: Comm, accum=None, slots_per_pixel: int = 0, profile: bool = False,
                     overwrite: bool = False):
        """Camera::render over all ranks of `comm` (pt_render_multi): spp sharding + one RCCL reduce onto rank 0.
        Returns (accum on rank 0 / None elsewhere, this rank's stats). ``overwrite``: the frame replaces ``accum``'s content
        instead of being added to it (a host that renders frame after frame into one buffer)."""
        h = image_height(cam)
        opts = RenderOpts(slots_per_pixel, 0, 1 if profile else 0, 1 if overwrite else 0, None)
        stats = RenderStats()
        ptr = None
        if comm.rank == 0:
            if accum is None:
                accum = np.zeros((h, cam.image_width, 3), dtype=np.float64)
            assert accum.dtype == np.float64 and accum.flags["C_CONTIGUOUS"] and accum.size == h * cam.image_width * 3
            ptr = C.c_void_p(accum.ctypes.data)
        _check(lib.pt_render_multi(self.handle, C.byref(cam), seed, spp_total, comm.handle, ptr, C.byref(opts), C.byref(stats)), "pt_render_multi")
        return (accum if comm.rank == 0 else None), stats

    def intersect(self, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 7)
        out = np.empty((len(rays), 15), dtype=np.float64)
        _check(lib.pt_intersect(self.handle, rays.ctypes.data, len(rays), out.ctypes.data), "pt_intersect")
        return out

    def env_probe(self, cam: Camera, which: int, arr: np.ndarray) -> np.ndarray:
        """The device functions of environment sampling for cam's environment map. which 0: arr = (n, 2) draws (u1, u2) ->
        (n, 4) {dir.xyz, pdf}; which 1: arr = (n, 3) directions -> (n,) env_pdf."""
        arr = np.ascontiguousarray(arr, dtype=np.float64).reshape(-1, 2 if which == 0 else 3)
        out = np.empty((len(arr), 4) if which == 0 else (len(arr),), dtype=np.float64)
        _check(lib.pt_env_probe(self.handle, C.byref(cam), which, arr.ctypes.data, len(arr), out.ctypes.data), "pt_env_probe")
        return out


# every non-HDR image a scene script opens (for hosts that decode everything themselves, e.g. the test oracle via Pillow)
SCENE_IMAGE_FILES = {2: ["earthmap.jpg"], 5: ["envmap.jpg"], 7: ["bricks/color.png", "bricks/normal.png"]}


def motion_pose(axis, angle0, angle1, tr0, tr1, time) -> np.ndarray:
    """The pose of a moving instance at `time` (pt_motion_pose; host only): 8 rows c0, c1, c2, t, i0, i1, i2, it."""
    out = (C.c_double * 24)()
    _check(lib.pt_motion_pose(_d3(axis), float(angle0), float(angle1), _d3(tr0), _d3(tr1), float(time), out), "pt_motion_pose")
    return np.array(out[:], dtype=np.float64).reshape(8, 3)


def motion_swept_box(box, axis, angle0, angle1, tr0, tr1) -> np.ndarray:
    """One level of the box rule of moving instances (pt_motion_swept_box; host only): box = (lo.xyz, hi.xyz) -> its box over times [0, 1]."""
    b = (C.c_double * 6)(*[float(x) for x in box])
    out = (C.c_double * 6)()
    _check(lib.pt_motion_swept_box(b, _d3(axis), float(angle0), float(angle1), _d3(tr0), _d3(tr1), out), "pt_motion_swept_box")
    return np.array(out[:], dtype=np.float64)


def punctual_eval(rec16, point) -> np.ndarray:
    """What a punctual light sends to a point (pt_punctual_eval; host only — the device's function compiled for the host): rec16 = a record as
    Scene.punctual_light returns it -> (w.xyz, D, E.rgb)."""
    rec = (C.c_double * 16)(*[float(x) for x in rec16])
    out = (C.c_double * 7)()
    _check(lib.pt_punctual_eval(rec, _d3(point), out), "pt_punctual_eval")
    return np.array(out[:], dtype=np.float64)


def _grid_args(box, dims):
    return np.ascontiguousarray(box, dtype=np.float64).reshape(6), np.ascontiguousarray(dims, dtype=np.uint32).reshape(3)


def punctual_grid_row(recs16, box, dims, cell) -> np.ndarray:
    """One row of the light grid's table (pt_punctual_grid_row; host only — the build kernel's functions compiled for the host): recs16 = (n, 16)
    records as Scene.punctual_light returns them, box = (lo.xyz, hi.xyz), dims = (nx, ny, nz) -> the cell's CDF C[0..n-1]."""
    recs = np.ascontiguousarray(recs16, dtype=np.float64).reshape(-1, 16)
    b, d = _grid_args(box, dims)
    out = np.empty(len(recs), dtype=np.float64)
    _check(lib.pt_punctual_grid_row(recs.ctypes.data, len(recs), b.ctypes.data, d.ctypes.data, int(cell), out.ctypes.data), "pt_punctual_grid_row")
    return out


def punctual_grid_select(box, dims, table, points, u) -> np.ndarray:
    """The light grid's selection (pt_punctual_grid_select; host only): table = (cells, n) the whole table, points (m, 3), u (m,) -> (m, 3)
    {cell, k, p}."""
    b, d = _grid_args(box, dims)
    table = np.ascontiguousarray(table, dtype=np.float64)
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
    if table.ndim != 2 or table.shape[0] != int(d[0]) * int(d[1]) * int(d[2]) or len(u) != len(points):
        raise PtError("punctual_grid_select: table is (nx * ny * nz, n), and there is one u per point")
    out = np.empty((len(points), 3), dtype=np.float64)
    _check(lib.pt_punctual_grid_select(b.ctypes.data, d.ctypes.data, table.ctypes.data, table.shape[1], points.ctypes.data, u.ctypes.data, len(points), out.ctypes.data),
           "pt_punctual_grid_select")
    return out


def sky_tiles(cam: Camera, boxes) -> np.ndarray:
    """The sky pass's tile test (pt_sky_tiles; host only): boxes (n, 6) = (lo.xyz, hi.xyz) -> (tiles_y, tiles_x) uint8, 1 = no camera ray
    of the 8x8 pixel tile can enter any box."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
    tiles_y, tiles_x = (image_height(cam) + 7) // 8, (cam.image_width + 7) // 8
    out = np.zeros((tiles_y, tiles_x), dtype=np.uint8)
    _check(lib.pt_sky_tiles(C.byref(cam), len(boxes), boxes.ctypes.data if len(boxes) else None, out.ctypes.data), "pt_sky_tiles")
    return out


def short_tiles(cam: Camera, boxes, shadeable) -> np.ndarray:
    """The tile test read per box (pt_short_tiles; host only): boxes (n, 6), shadeable (n,) flags -> (tiles_y, tiles_x) uint8, 1 = sure sky,
    2 = short (every box the test cannot clear is shadeable), 0 = the path pool's."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
    flags = np.ascontiguousarray(shadeable, dtype=np.uint8).reshape(-1)
    assert len(flags) == len(boxes)
    tiles_y, tiles_x = (image_height(cam) + 7) // 8, (cam.image_width + 7) // 8
    out = np.zeros((tiles_y, tiles_x), dtype=np.uint8)
    _check(lib.pt_short_tiles(C.byref(cam), len(boxes), boxes.ctypes.data if len(boxes) else None, flags.ctypes.data if len(boxes) else None, out.ctypes.data),
           "pt_short_tiles")
    return out


def tile_reach(cam: Camera, boxes) -> np.ndarray:
    """The tile test's answer per box (pt_tile_reach; host only): boxes (n, 6) -> (tiles_y, tiles_x) uint64, bit b = 0: no camera ray of the tile
    enters box b; all ones where the test says nothing."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
    tiles_y, tiles_x = (image_height(cam) + 7) // 8, (cam.image_width + 7) // 8
    out = np.zeros((tiles_y, tiles_x), dtype=np.uint64)
    _check(lib.pt_tile_reach(C.byref(cam), len(boxes), boxes.ctypes.data if len(boxes) else None, out.ctypes.data), "pt_tile_reach")
    return out


def camera_init(cam: Camera):
    """Camera::init (camera.rs:51-77) -> (dict of derived vectors, image_height)."""
    out = (C.c_double * 18)()
    h = C.c_uint32()
    _check(lib.pt_camera_init(C.byref(cam), out, C.byref(h)), "pt_camera_init")
    v = np.array(out).reshape(6, 3)
    names = ["forward", "right", "up", "pixel00", "pixel_du", "pixel_dv"]
    return {n: v[i] for i, n in enumerate(names)}, h.value


def image_height(cam: Camera) -> int:
    return camera_init(cam)[1]


def load_obj(path: str):
    pos, idx, uv = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)()
    npos, nidx, nuv = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib.pt_load_obj(path.encode(), C.byref(pos), C.byref(npos), C.byref(idx), C.byref(nidx), C.byref(uv), C.byref(nuv)), "pt_load_obj")
    P = np.ctypeslib.as_array(pos, (npos.value * 3,)).copy().reshape(-1, 3) if npos.value else np.zeros((0, 3), np.float32)
    I = np.ctypeslib.as_array(idx, (nidx.value,)).copy() if nidx.value else np.zeros(0, np.uint32)
    T = np.ctypeslib.as_array(uv, (nuv.value * 2,)).copy().reshape(-1, 2) if nuv.value else np.zeros((0, 2), np.float32)
    lib.pt_free(pos); lib.pt_free(idx); lib.pt_free(uv)
    return P, I, T


def load_obj_single_index(path: str):
    """OBJ with vn / separate index streams -> (positions, indices, normals | None, texcoords | None), one index per corner."""
    pos, idx, nrm, uv = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
    npos, nidx, nnrm, nuv = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib.pt_load_obj_single_index(path.encode(), C.byref(pos), C.byref(npos), C.byref(idx), C.byref(nidx), C.byref(nrm), C.byref(nnrm),
                                        C.byref(uv), C.byref(nuv)), "pt_load_obj_single_index")
    arr = lambda p, n, k, dt: np.ctypeslib.as_array(p, (n * k,)).copy().reshape(-1, k) if n else None
    out = (arr(pos, npos.value, 3, np.float32), np.ctypeslib.as_array(idx, (nidx.value,)).copy() if nidx.value else np.zeros(0, np.uint32),
           arr(nrm, nnrm.value, 3, np.float32), arr(uv, nuv.value, 2, np.float32))
    for p in (pos, idx, nrm, uv):
        lib.pt_free(p)
    return out


def load_jpeg_rgb8(path: str) -> np.ndarray:
    """Baseline / progressive JPEG -> RGB8 by the library's own decoder (csrc/pt_jpeg.cpp)."""
    p = C.POINTER(C.c_uint8)()
    w, h = C.c_uint32(), C.c_uint32()
    _check(lib.pt_load_jpeg_rgb8(path.encode(), C.byref(p), C.byref(w), C.byref(h)), "pt_load_jpeg_rgb8")
    img = np.ctypeslib.as_array(p, (h.value, w.value, 3)).copy()
    lib.pt_free(p)
    return img


def load_png_rgb8(path: str) -> np.ndarray:
    p = C.POINTER(C.c_uint8)()
    w, h = C.c_uint32(), C.c_uint32()
    _check(lib.pt_load_png_rgb8(path.encode(), C.byref(p), C.byref(w), C.byref(h)), "pt_load_png_rgb8")
    img = np.ctypeslib.as_array(p, (h.value, w.value, 3)).copy()
    lib.pt_free(p)
    return img


def load_hdr_rgbf32(path: str) -> np.ndarray:
    """Radiance .hdr -> f32 RGB (the decode of texture.rs:62-66 WITHOUT .to_rgb8())."""
    p = C.POINTER(C.c_float)()
    w, h = C.c_uint32(), C.c_uint32()
    _check(lib.pt_load_hdr_rgbf32(path.encode(), C.byref(p), C.byref(w), C.byref(h)), "pt_load_hdr_rgbf32")
    img = np.ctypeslib.as_array(p, (h.value, w.value, 3)).copy()
    lib.pt_free(p)
    return img


def load_hdr_rgb8(path: str) -> np.ndarray:
    p = C.POINTER(C.c_uint8)()
    w, h = C.c_uint32(), C.c_uint32()
    _check(lib.pt_load_hdr_rgb8(path.encode(), C.byref(p), C.byref(w), C.byref(h)), "pt_load_hdr_rgb8")
    img = np.ctypeslib.as_array(p, (h.value, w.value, 3)).copy()
    lib.pt_free(p)
    return img


def save_png(path: str, rgb8: np.ndarray):
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w = rgb8.shape[:2]
    _check(lib.pt_save_png(path.encode(), w, h, rgb8.ctypes.data), "pt_save_png")


def _save_f32(fn, what: str, path: str, rgb: np.ndarray):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[:2]
    assert rgb.shape == (h, w, 3)
    _check(fn(path.encode(), w, h, rgb.ctypes.data), what)


def save_hdr(path: str, rgb: np.ndarray):
    """(H, W, 3) float image -> Radiance RGBE .hdr (pt_save_hdr; load_hdr_rgbf32 reads it back)."""
    _save_f32(lib.pt_save_hdr, "pt_save_hdr", path, rgb)


def save_pfm(path: str, rgb: np.ndarray):
    """(H, W, 3) float image -> little-endian colour .pfm, the f32 bits as they are (pt_save_pfm)."""
    _save_f32(lib.pt_save_pfm, "pt_save_pfm", path, rgb)
