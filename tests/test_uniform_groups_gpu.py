"""Single-primitive groups and the sphere (u, v) flag of k_shade.

A group of k_shade whose surface lanes all hit ONE sphere or quad reads its PrimRef, instance chain, primitive record, material
fields and texture descriptor through scalar loads; every other group gathers them per lane. A sphere's (u, v) is computed only
where the scene build set PRIM_NEEDS_UV (pt_types.h): a normal map, an image texture in the colour tree, or a mix with such a
child. Neither changes an operand, so every render here must equal the oracle's bit for bit (static mode, one slot per pixel,
deterministic math), and the dynamic mode must equal its in-place form as in test_shading_order_gpu.py. Each scene is chosen
because one of the two can go wrong there."""
import os

import numpy as np
import pytest

from common import SceneSpec, default_camera

pytestmark = pytest.mark.gpu

W, ASPECT = 64, 16.0 / 9.0     # 64 x 36 pixels: 36 groups of 64 slots


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def _camera(**kw):
    cam = dict(width=W, aspect=ASPECT, spp=8, env_color=(0.6, 0.7, 0.9))
    cam.update(kw)
    return default_camera(**cam)


def _assert_bit_exact(pt, det, ctx, spec, seed=3, spp=8):
    gs, os_ = pt.Scene(ctx), det.Scene()
    gres, ores = spec.replay(gs), spec.replay(os_)
    assert gs.prim_count() == os_.prim_count()
    ga, st = gs.render(spec.make_camera(pt.Camera, gres), seed, 0, spp, slots_per_pixel=1)
    oa, cnt = os_.render(spec.make_camera(det.Camera, ores), seed, 0, spp)
    gs.close(); os_.close()
    assert ga.shape[:2] == (36, 64)
    assert st.segments == cnt["segments"] and st.samples == cnt["samples"] == ga.shape[0] * ga.shape[1] * spp
    np.testing.assert_array_equal(ga, oa)
    assert np.isfinite(ga).mean() > 0.99 and ga[np.isfinite(ga)].max() > 0
    return ga, st


def _env_image(seed):
    return np.random.default_rng(seed).integers(0, 256, (32, 64, 3), dtype=np.uint8)


def test_frame_filling_flat_checker_quad_under_an_environment_map(pt, det, ctx):
    """Every surface group is one quad: PrimRef, QuadD, the material and the flat checker's descriptor all come by scalar loads."""
    spec = SceneSpec()
    rgb = lambda r, g, b: spec.add("tex_solid_rgb", r, g, b)
    ground = spec.add("mat_diffuse", spec.add("tex_checker", 0.7, rgb(0.2, 0.3, 0.1), rgb(0.9, 0.9, 0.9)), -1)
    spec.add("world_add_object", spec.add("quad", (-40.0, 0.0, -40.0), (0.0, 0.0, 80.0), (80.0, 0.0, 0.0), ground))
    env = spec.add("tex_image_rgb8", _env_image(1))
    spec.add("world_build")
    spec.camera = _camera(look_from=(0.0, 3.0, -4.0), look_at=(0.0, 0.0, 0.0), env_is_map=1, env_tex=env)
    ga, st = _assert_bit_exact(pt, det, ctx, spec)
    assert st.segments == 2 * st.samples      # the quad fills the frame: every path is one hit and one miss


def _three_spheres(pt, spec):
    rgb = lambda r, g, b: spec.add("tex_solid_rgb", r, g, b)
    earth = pt.decode_image_rgb8(os.path.join(pt.ASSET_DIR, "earthmap.jpg"))
    metal = spec.add("mat_metal", rgb(0.7, 0.6, 0.5), spec.add("tex_solid_f", 0.1))
    glass = spec.add("mat_glass", rgb(1.0, 1.0, 1.0), spec.add("tex_solid_f", 0.02), 0.0, 1.5)
    globe = spec.add("mat_diffuse", spec.add("tex_image_rgb8", earth), -1)
    for x, m in ((-2.1, metal), (0.0, glass), (2.1, globe)):
        spec.add("world_add_object", spec.add("sphere", 1.0, (x, 1.0, 0.0), (x, 1.0, 0.0), m))


def test_solid_and_image_textured_spheres_in_one_window(pt, det, ctx):
    """PRIM_NEEDS_UV clear (solid metal, solid glass) and set (the earth map on a diffuse sphere) in the same window."""
    spec = SceneSpec()
    _three_spheres(pt, spec)
    spec.add("world_build")
    spec.camera = _camera(look_from=(0.0, 1.2, -5.5), look_at=(0.0, 1.0, 0.0), vfov=45.0)
    _assert_bit_exact(pt, det, ctx, spec)


def test_sphere_with_a_normal_map_and_a_solid_colour(pt, det, ctx):
    """The flag must be set by the normal map alone: the colour is solid, finish_hit reads the map at (u, v)."""
    rng = np.random.default_rng(5)
    nmap = np.clip(rng.normal(128, 40, (16, 32, 3)), 0, 255).astype(np.uint8); nmap[..., 2] = 255
    spec = SceneSpec()
    m = spec.add("mat_diffuse", spec.add("tex_solid_rgb", 0.7, 0.6, 0.5), spec.add("tex_image_rgb8", nmap))
    spec.add("world_add_object", spec.add("sphere", 1.5, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), m))
    spec.add("world_build")
    spec.camera = _camera(look_from=(0.0, 1.2, -4.0), look_at=(0.0, 1.0, 0.0))
    _assert_bit_exact(pt, det, ctx, spec)


def test_spheres_of_mixes_with_an_image_textured_child(pt, det, ctx):
    """The host rule is transitive: a mix with an image-textured child, and one with that mix as its child; next to them a mix of
    solid leaves, whose sphere keeps the flag clear."""
    rng = np.random.default_rng(6)
    spec = SceneSpec()
    rgb = lambda r, g, b: spec.add("tex_solid_rgb", r, g, b)
    img = spec.add("tex_image_rgb8", rng.integers(0, 256, (16, 32, 3), dtype=np.uint8))
    textured = spec.add("mat_diffuse", spec.add("tex_checker", 0.4, img, rgb(0.9, 0.2, 0.2)), -1)   # the image sits under a checker
    coat = spec.add("mat_clearcoat", 0.7)
    metal = spec.add("mat_metal", rgb(0.8, 0.8, 0.6), spec.add("tex_solid_f", 0.2))
    plain = spec.add("mat_diffuse", rgb(0.3, 0.5, 0.7), -1)
    mix1 = spec.add("mat_mix", 0.4, textured, coat)
    mix2 = spec.add("mat_mix", 0.6, metal, mix1)
    mix0 = spec.add("mat_mix", 0.5, plain, metal)
    for x, m in ((-2.1, mix1), (0.0, mix2), (2.1, mix0)):
        spec.add("world_add_object", spec.add("sphere", 1.0, (x, 1.0, 0.0), (x, 1.0, 0.0), m))
    spec.add("world_add_light", spec.add("quad", (-1.5, 4.0, -1.5), (3.0, 0.0, 0.0), (0.0, 0.0, 3.0), spec.add("mat_light", rgb(7.0, 7.0, 6.0))))
    spec.add("world_build")
    spec.camera = _camera(look_from=(0.0, 1.2, -5.5), look_at=(0.0, 1.0, 0.0), vfov=45.0, env_color=(0.05, 0.05, 0.08))
    _assert_bit_exact(pt, det, ctx, spec)


def test_sphere_and_quad_under_two_rotated_instances(pt, det, ctx):
    """The uniform path with an instance chain: ray_to_local_chain<true> and the way back to world space, for both kinds."""
    spec = SceneSpec()
    rgb = lambda r, g, b: spec.add("tex_solid_rgb", r, g, b)
    ground = spec.add("mat_diffuse", spec.add("tex_checker", 0.9, rgb(0.2, 0.3, 0.1), rgb(0.9, 0.9, 0.9)), -1)
    metal = spec.add("mat_metal", rgb(0.8, 0.7, 0.5), spec.add("tex_solid_f", 0.15))
    q = spec.add("quad", (-40.0, 0.0, -40.0), (0.0, 0.0, 80.0), (80.0, 0.0, 0.0), ground)
    q = spec.add("instance", q, (0.0, 1.0, 0.0), 0.4, (0.5, 0.0, 0.0))
    spec.add("world_add_object", spec.add("instance", q, (1.0, 0.0, 0.0), 0.05, (0.0, -0.2, 0.3)))
    b = spec.add("sphere", 1.6, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), metal)
    b = spec.add("instance", b, (0.0, 0.0, 1.0), 0.7, (0.2, 1.0, 0.0))
    spec.add("world_add_object", spec.add("instance", b, (0.0, 1.0, 0.0), -0.5, (0.0, 0.8, 0.4)))
    spec.add("world_build")
    spec.camera = _camera(look_from=(0.0, 2.5, -5.0), look_at=(0.0, 1.2, 0.0))
    _assert_bit_exact(pt, det, ctx, spec)


def _cuboid_next_to_quad():
    """A cuboid under an instance next to a quad of the same material class: six gids and the quad's in one class — mixed groups,
    which must fall back to the per-lane path, between uniform ones."""
    spec = SceneSpec()
    rgb = lambda r, g, b: spec.add("tex_solid_rgb", r, g, b)
    ground = spec.add("mat_diffuse", spec.add("tex_checker", 0.7, rgb(0.25, 0.2, 0.3), rgb(0.9, 0.9, 0.85)), -1)
    red = spec.add("mat_diffuse", rgb(0.8, 0.2, 0.15), -1)
    spec.add("world_add_object", spec.add("quad", (-20.0, 0.0, -20.0), (0.0, 0.0, 40.0), (40.0, 0.0, 0.0), ground))
    box = spec.add("cuboid", (-1.0, 0.0, -1.0), (1.0, 2.0, 1.0), red)
    spec.add("world_add_object", spec.add("instance", box, (0.0, 1.0, 0.0), 0.6, (0.3, 0.0, 0.5)))
    spec.add("world_build")
    spec.camera = _camera(look_from=(0.0, 2.5, -6.0), look_at=(0.0, 0.8, 0.0))
    return spec


def test_cuboid_under_an_instance_next_to_a_quad_of_the_same_class(pt, det, ctx):
    _assert_bit_exact(pt, det, ctx, _cuboid_next_to_quad())


@pytest.mark.parametrize("which", ["cuboid_and_quad", "scene6"])
def test_dynamic_mode_equals_in_place(pt, ctx, which):
    """Groups with bystander lanes and windows with a single surface lane: the dynamic mode on small pools against its in-place
    form. Which slot a path sits in decides nothing, so sample and segment counts are equal and the sums agree up to the order of
    the f64 atomics (1e-12 relative: the tolerance of test_shading_order_gpu.py)."""
    spp = 16
    gs = pt.Scene(ctx)
    if which == "scene6":
        cam = gs.build_scene(6, 64, spp)
    else:
        spec = _cuboid_next_to_quad()
        cam = spec.make_camera(pt.Camera, spec.replay(gs))
    for pool in ("4096", "70000"):
        env = {"PT_EXPERIMENT": "1", "PT_POOL_SLOTS": pool}
        ordered, st = _with_env(env, lambda: gs.render(cam, 3, 0, spp))
        in_place, st_ip = _with_env(dict(env, PT_POOL_IN_PLACE="1"), lambda: gs.render(cam, 3, 0, spp))
        assert st.samples == st_ip.samples == ordered.shape[0] * ordered.shape[1] * spp, (pool, st.samples, st_ip.samples)
        assert st.segments == st_ip.segments, (pool, st.segments, st_ip.segments)
        fin = np.isfinite(in_place)
        assert (np.isfinite(ordered) == fin).all(), pool
        np.testing.assert_allclose(ordered[fin], in_place[fin], rtol=1e-12, atol=0.0, err_msg=f"{which} pool {pool}")
    gs.close()


def test_probe_still_reports_uv_of_a_solid_sphere(pt, det, ctx):
    """k_probe keeps the full computation: (u, v) of a sphere whose PRIM_NEEDS_UV is clear equal the oracle's."""
    spec = SceneSpec()
    m = spec.add("mat_metal", spec.add("tex_solid_rgb", 0.7, 0.6, 0.5), spec.add("tex_solid_f", 0.1))
    spec.add("world_add_object", spec.add("sphere", 1.0, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), m))
    spec.add("world_build")
    gs, os_ = pt.Scene(ctx), det.Scene()
    spec.replay(gs); spec.replay(os_)
    rng = np.random.default_rng(8)
    rays = np.zeros((512, 7))
    rays[:, 0:3] = (0.0, 1.0, -5.0)
    rays[:, 3:6] = rng.normal(size=(512, 3)) * 0.12 + (0.0, 0.0, 1.0)
    g = gs.intersect(rays)
    np.testing.assert_array_equal(g, os_.intersect(rays))
    hit = g[:, 0] > 0
    assert hit.sum() > 200 and (g[hit, 3] > 0).all() and (g[hit, 4] > 0).all() and g[hit, 3].std() > 0.01
    gs.close(); os_.close()
