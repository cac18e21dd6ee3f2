"""Camera projections (pt_scene_set_projection) on the GPU: the ray generator against the numpy restatement of the rule
(tests/camera_rule.py) bit for bit, renders and AOVs against the probe's rays, and tests of each projection's geometry that do not use
the restatement: a panorama of an environment map gives the map back, orthographic discs do not shrink with depth, and the fisheye
puts a direction at theta off axis at theta / th of the half height."""
import os
import subprocess

import numpy as np
import pytest

import camera_rule as CR
import sampler_rule as R
from common import SceneSpec, _with_env, default_camera, shared_and_nested_instances_scene

pytestmark = pytest.mark.gpu

SEEDS = (1, (9 << 32) | 4)                       # one above 2^32
SAMPLERS = ("independent", "sobol")


def camera_of(pt, **kw):
    spec = SceneSpec()
    spec.camera = default_camera(**kw)
    return spec.make_camera(pt.Camera, [])


# ---- 1. the probe against the rule ---------------------------------------------------------------------------------------------------
PROBE_CAM = dict(width=16, aspect=2.0, vfov=120.0, blur_strength=0.5, look_from=(0.3, 1.0, -6.0), look_at=(-0.2, 0.4, 0.5), vup=(0.1, 1.0, 0.0),
                 focal_length=5.5)                # 16 x 8; a fisheye corner at sqrt(5) * 60 = 134 degrees
PROBE_CASES = [(0, 0.0), (0, 1.5), (1, 0.0), (1, 1.5), (2, 0.0), (3, 0.0)]


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("kind, defocus", PROBE_CASES)
def test_probe_is_the_numpy_rule_bit_for_bit(pt, ctx, kind, defocus, sampler):
    cam = camera_of(pt, defocus_angle=defocus, **PROBE_CAM)
    frame, h = pt.camera_init(cam)
    assert h == 8
    gs = pt.Scene(ctx)                            # no world: time is drawn
    gs.set_projection(kind)
    gs.set_sampler(sampler)
    assert gs.projection() == kind
    pixels = np.repeat(np.arange(16 * 8), 4)
    samples = np.tile(np.arange(4), 16 * 8)
    for seed in SEEDS:
        got = gs.camera_probe(cam, seed, np.stack([pixels, samples], axis=1))
        o, d, t, n = CR.camera_rays(kind, frame, h, cam, seed, pixels, samples, sobol=sampler == "sobol")
        np.testing.assert_array_equal(got[:, 0:3], o)
        np.testing.assert_array_equal(got[:, 3:6], d)
        np.testing.assert_array_equal(got[:, 6], t)
        np.testing.assert_array_equal(got[:, 7], float(n))
        assert n == 5 and (t > 0.0).any()
        if kind == 0 and defocus == 0.0:          # the rule that predates the probe: image-plane locations by libm's cos / sin
            fy, fx = R.camera_locations(frame, PROBE_CAM["blur_strength"], 16, seed, np.arange(16 * 8), np.arange(4), sobol=sampler == "sobol")
            S = frame["pixel00"] + frame["pixel_dv"] * fy.reshape(-1, 1) + frame["pixel_du"] * fx.reshape(-1, 1)
            w = S - np.array(PROBE_CAM["look_from"])
            np.testing.assert_allclose(got[:, 3:6], w / np.linalg.norm(w, axis=1)[:, None], rtol=0.0, atol=1e-13)
            np.testing.assert_array_equal(got[:, 0:3], np.broadcast_to(PROBE_CAM["look_from"], (len(got), 3)))
    with pytest.raises(pt.PtError):               # a pixel outside the frame
        gs.camera_probe(cam, 1, np.array([[16 * 8, 0]]))
    gs.close()


# ---- 2. renders and AOVs trace the probe's rays ------------------------------------------------------------------------------------
# test_sampler_gpu's scene: one emissive quad, nothing else, a black environment: a sample's radiance is the emission if its camera
# ray hits the quad and 0 otherwise, so a pixel's sum is emission * (number of its camera rays that hit).
QUAD_Q, QUAD_U, QUAD_V = (-0.9, -0.6, 0.0), (1.6, 0.5, 0.0), (-0.4, 1.5, 0.0)
QUAD_EMISSION = (2.0, 1.0, 0.5)                  # powers of two: emission * count is exact
COUNT_SPP = 8
COUNT_CAMS = {1: dict(width=32, aspect=1.0, look_from=(0.0, 0.0, -5.0), focal_length=5.0, vfov=40.0),
              2: dict(width=32, aspect=1.0, look_from=(0.0, 0.0, -5.0), focal_length=5.0, vfov=40.0),
              3: dict(width=64, aspect=2.0, look_from=(0.0, 0.0, -1.2), focal_length=1.2, vfov=40.0)}


def quad_scene(pt, ctx, kind):
    spec = SceneSpec()
    lm = spec.add("mat_light", spec.add("tex_solid_rgb", *QUAD_EMISSION))
    spec.add("world_add_object", spec.add("quad", QUAD_Q, QUAD_U, QUAD_V, lm))
    spec.add("world_build")
    spec.camera = default_camera(spp=COUNT_SPP, max_depth=8, look_at=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), defocus_angle=0.0, blur_strength=0.5,
                                 env_color=(0.0, 0.0, 0.0), **COUNT_CAMS[kind])
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    gs.set_projection(kind)
    return gs, cam


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_renders_and_aovs_trace_the_probe_rays(pt, ctx, kind, sampler):
    gs, cam = quad_scene(pt, ctx, kind)
    gs.set_sampler(sampler)
    w, h = cam.image_width, pt.image_height(cam)
    spp, seed = COUNT_SPP, SEEDS[1]
    pixels = np.repeat(np.arange(w * h), spp)
    samples = np.tile(np.arange(spp), w * h)
    rays = gs.camera_probe(cam, seed, np.stack([pixels, samples], axis=1))
    assert (rays[:, 6] == 0.0).all() and (rays[:, 7] == 5.0).all()          # nothing moves: the time draw is made by index only
    count = gs.intersect(rays[:, :7])[:, 0].reshape(w * h, spp).sum(axis=1)
    assert (count == spp).any() and (count == 0).any() and ((count > 0) & (count < spp)).any()
    aov = gs.render_aovs(cam, seed, 0, spp)
    np.testing.assert_array_equal(aov.reshape(w * h, 8)[:, 7], count)
    expected = count[:, None] * np.array(QUAD_EMISSION)
    acc, st = gs.render(cam, seed, 0, spp, slots_per_pixel=1)                # K1 only: every sample's ray comes from k_init
    np.testing.assert_array_equal(acc.reshape(w * h, 3), expected)
    assert st.samples == w * h * spp
    for env in ({}, {"PT_EXPERIMENT": "1", "PT_POOL_SLOTS": "1000"}):        # dynamic pools; the small one regenerates in k_shade
        dyn, st = _with_env(env, lambda: gs.render(cam, seed, 0, spp))
        assert st.samples == w * h * spp, env
        if env:
            assert st.n_slots == 1000
        np.testing.assert_allclose(dyn.reshape(w * h, 3), expected, rtol=1e-11, atol=1e-11, err_msg=str(env))
    gs.close()


# ---- 3. pixel lists and adaptive sampling ----------------------------------------------------------------------------------------------
def test_pixel_lists_and_adaptive_under_a_panorama(pt, ctx):
    spec = shared_and_nested_instances_scene()                               # meshes under instances, a light list
    spec.camera = dict(spec.camera, aspect_ratio=2.0, defocus_angle=0.0, samples_per_pixel=4)
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    gs.set_projection("panorama")
    w, h = 64, pt.image_height(cam)
    assert h == 32
    whole, _ = gs.render(cam, 5, 0, 4, slots_per_pixel=1)
    listed = np.sort(np.random.default_rng(3).choice(w * h, size=100, replace=False))
    sentinel = -7.25
    part, st = gs.render_pixels(cam, 5, listed, 0, 4, accum=np.full((h, w, 3), sentinel), slots_per_pixel=1, overwrite=True)
    assert st.samples == 100 * 4
    mask = np.zeros(w * h, dtype=bool)
    mask[listed] = True
    np.testing.assert_array_equal(part.reshape(-1, 3)[mask], whole.reshape(-1, 3)[mask])
    assert (part.reshape(-1, 3)[~mask] == sentinel).all()
    persp = pt.Scene(ctx)                                                     # (the setting acts: the perspective frame differs)
    spec.replay(persp)
    other, _ = persp.render(cam, 5, 0, 4, slots_per_pixel=1)
    assert not np.array_equal(other, whole)
    persp.close()
    acc, counts, st = gs.render_adaptive(cam, 5, 4, 16, 0.05)
    assert int(counts.sum()) == st.samples and counts.min() >= 4 and counts.max() <= 16
    assert np.isfinite(acc).all()
    gs.close()


# ---- 4. the panorama of an environment map is the map (independent of camera_rule) -----------------------------------------------------
def test_panorama_gives_the_environment_map_back(pt, ctx):
    W, H, spp = 64, 32, 4
    env_img = np.random.default_rng(17).uniform(0.0, 4.0, size=(H, W, 3)).astype(np.float32)
    center = np.array([0.5, 1.0, -2.0])
    # pixel-centre directions, straight from the header's formulas
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    phi = -np.pi + ((2.0 * np.pi) * (i + 0.5)) / W
    theta = (np.pi * (j + 0.5)) / H
    d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1)
    ball_c, ball_r = center + 10.0 * d[12, 40], 0.05                         # pt_world_build refuses an empty world: one small far sphere
    spec = SceneSpec()
    env = spec.add("tex_image_rgbf32", env_img)
    grey = spec.add("mat_diffuse", spec.add("tex_solid_rgb", 0.5, 0.5, 0.5), -1)
    spec.add("world_add_object", spec.add("sphere", ball_r, tuple(ball_c), tuple(ball_c), grey))
    spec.add("world_build")
    spec.camera = default_camera(width=W, aspect=2.0, spp=spp, look_from=tuple(center), look_at=(0.0, 0.5, 0.0), defocus_angle=0.0, blur_strength=0.0,
                                 env_is_map=1, env_tex=env)
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    gs.set_projection("panorama")
    # ray-sphere discriminant of the centre directions, grown by the 8 neighbours
    oc = center - ball_c
    b = d @ oc
    meets = (b * b - (oc @ oc - ball_r * ball_r) >= 0.0) & (b < 0.0)
    assert meets[12, 40]
    out = meets.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out |= np.roll(np.roll(meets, dy, axis=0), dx, axis=1)
    print(f"panorama identity: {int(meets.sum())} pixel centres meet the sphere, {int(out.sum())} pixels left out")
    assert out.sum() <= 12
    expected = float(spp) * env_img.astype(np.float64)
    for slots in (1, 0):
        for sampler in SAMPLERS:
            gs.set_sampler(sampler)
            acc, st = gs.render(cam, 3, 0, spp, slots_per_pixel=slots)
            np.testing.assert_array_equal(acc[~out], expected[~out])
    assert not np.array_equal(acc[12, 40], expected[12, 40])                # (the sphere is seen where it was put)
    gs.close()


# ---- 5. orthographic: size does not depend on depth (independent of camera_rule) ------------------------------------------------------
def test_orthographic_discs_do_not_shrink_with_depth(pt, ctx):
    W = 48
    camkw = dict(width=W, aspect=1.0, spp=1, vfov=40.0, look_from=(0.0, 0.0, -5.0), look_at=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), focal_length=5.0,
                 defocus_angle=0.0, blur_strength=0.0, env_color=(0.0, 0.0, 0.0))
    frame, h = pt.camera_init(camera_of(pt, **camkw))
    assert h == W
    du, dv, p00, fwd = frame["pixel_du"], frame["pixel_dv"], frame["pixel00"], frame["forward"]
    px = np.linalg.norm(du)
    radius, shift = 0.5, 22                                                  # 6.6 pixels; the second disc 22 whole columns to the right
    row0, col0 = 23.3, 12.4                                                  # centres off the pixel grid: no pixel centre on a rim
    S1 = p00 + dv * row0 + du * col0                                         # on the focal plane, at depth F = 5
    c1, c2 = S1 + fwd * 2.0, S1 + du * shift - fwd * 4.0                     # depths 3 and 9 (the view direction is -forward)
    spec = SceneSpec()
    grey = spec.add("mat_diffuse", spec.add("tex_solid_rgb", 0.5, 0.5, 0.5), -1)
    for c in (c1, c2):
        spec.add("world_add_object", spec.add("sphere", radius, tuple(c), tuple(c), grey))
    spec.add("world_build")
    spec.camera = default_camera(**camkw)
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))

    def discs():
        hits = gs.render_aovs(cam, 1, 0, 1)[..., 7]
        assert set(np.unique(hits)) <= {0.0, 1.0}
        return hits[:, : W // 2] == 1.0, hits[:, W // 2:] == 1.0             # the discs lie in the left and the right half

    gs.set_projection("orthographic")
    left, right = discs()
    rows, cols = np.meshgrid(np.arange(W), np.arange(W), indexing="ij")
    dist1 = np.hypot(rows - row0, cols - col0) * px                          # pixel centres against the disc's centre, on the image plane
    dist2 = np.hypot(rows - row0, cols - (col0 + shift)) * px
    for mask, dist, half in ((left, dist1[:, : W // 2], "left"), (right, dist2[:, W // 2:], "right")):
        keep = np.abs(dist - radius) > 1e-9 * radius
        n_disc = int((dist < radius).sum())
        print(f"orthographic {half} disc: {n_disc} pixels, {int((~keep).sum())} left out at the rim")
        assert (~keep).sum() <= 0.01 * n_disc and n_disc > 100
        np.testing.assert_array_equal(mask[keep], (dist < radius)[keep])
    near, far = np.zeros((W, W), dtype=bool), np.zeros((W, W), dtype=bool)
    near[:, : W // 2], far[:, W // 2:] = left, right
    off_rim = np.abs(dist2 - radius) > 1e-9 * radius                         # (dist2 is dist1 moved by the shift)
    np.testing.assert_array_equal(np.roll(near, shift, axis=1)[off_rim], far[off_rim])       # the near disc moved onto the far one
    gs.set_projection("perspective")                                         # the same scene in perspective: the far disc is smaller
    pl, pr = discs()
    print(f"perspective discs: {int(pl.sum())} and {int(pr.sum())} pixels; orthographic: {int(left.sum())} and {int(right.sum())}")
    assert pl.sum() > 1.5 * left.sum() and pr.sum() < 0.5 * right.sum()
    gs.close()


# ---- 6. fisheye: the angle law (independent of camera_rule) ----------------------------------------------------------------------------
def test_fisheye_angle_law(pt, ctx):
    W = H = 48
    spp = 16
    spec = SceneSpec()
    lm = spec.add("mat_light", spec.add("tex_solid_rgb", 1.0, 1.0, 1.0))
    # the camera looks along -z from the origin: forward = (0, 0, 1), right = (1, 0, 0), up = (0, 1, 0)
    angles = (0.0, 30.0, 60.0)
    for a in angles:
        c = 10.0 * np.array([np.sin(np.radians(a)), 0.0, -np.cos(np.radians(a))])
        spec.add("world_add_object", spec.add("sphere", 1.0, tuple(c), tuple(c), lm))          # 5.7 degrees of angular radius: 1.5 pixels
    spec.add("world_build")
    spec.camera = default_camera(width=W, aspect=1.0, spp=spp, vfov=180.0, look_from=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), vup=(0.0, 1.0, 0.0),
                                 focal_length=1.0, defocus_angle=0.0, blur_strength=0.5, env_color=(0.0, 0.0, 0.0))
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    frame, h = pt.camera_init(cam)
    np.testing.assert_allclose(np.stack([frame["forward"], frame["right"], frame["up"]]), [[0, 0, 1], [1, 0, 0], [0, 1, 0]], atol=1e-15)
    gs.set_projection("fisheye")
    for sampler in SAMPLERS:
        gs.set_sampler(sampler)
        hits = gs.render_aovs(cam, 2, 0, spp)[..., 7]
        rows, cols = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")      # a pixel's centre in edge coordinates: index + 0.5
        windows = ((20, 28), (28, 36), (36, 44))                                              # columns around 24, 32 and 40
        assert hits[:, :20].sum() == 0 and hits[:, 44:].sum() == 0
        for a, (lo, hi) in zip(angles, windows):
            wgt = hits[:, lo:hi]
            assert wgt.sum() >= 4 * spp
            col = (wgt * cols[:, lo:hi]).sum() / wgt.sum()
            row = (wgt * rows[:, lo:hi]).sum() / wgt.sum()
            want = W / 2 + (a / 90.0) * H / 2
            print(f"fisheye {sampler}: sphere at {a} degrees: centroid column {col:.3f} (law: {want}), row {row:.3f} (law: {H / 2})")
            assert abs(col - want) < 0.5 and abs(row - H / 2) < 0.5
    gs.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_way_back(pt, ctx):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 64, 4)
    h = pt.image_height(cam)
    assert gs.projection() == 0
    for bad in (4, -1, 17, "cylindrical", None, 1.0):
        gs.set_projection("fisheye")
        with pytest.raises(pt.PtError):
            gs.set_projection(bad)
        assert gs.projection() == 2                                              # the setting is kept
    assert pt.lib.pt_scene_set_projection(gs.handle, 4) == -1 and b"kind must be" in pt.lib.pt_last_error()
    sentinel = 3.5

    def refused(match, **fields):
        c = pt.Camera.from_buffer_copy(cam)
        for k, v in fields.items():
            setattr(c, k, v)
        acc = np.full((pt.image_height(c), c.image_width, 3), sentinel)
        with pytest.raises(pt.PtError, match=match):
            gs.render(c, 1, 0, 4, accum=acc)
        assert (acc == sentinel).all()
        with pytest.raises(pt.PtError, match=match):
            gs.render(c, 1, 0, 4, accum=acc, slots_per_pixel=1)
        aov = np.full((pt.image_height(c), c.image_width, 8), sentinel)
        with pytest.raises(pt.PtError, match=match):
            gs.render_aovs(c, 1, 0, 4, aov=aov)
        assert (acc == sentinel).all() and (aov == sentinel).all()
        with pytest.raises(pt.PtError, match=match):
            gs.camera_probe(c, 1, np.array([[0, 0]]))

    for kind in ("fisheye", "panorama"):
        gs.set_projection(kind)
        refused("defocus_angle", defocus_angle=1.0)
    gs.set_projection("fisheye")
    refused("image circle", vfov=300.0)                                          # aspect 1: the corner would be at sqrt(2) * 150 degrees
    refused("vfov", vfov=float("inf"))
    gs.set_projection("orthographic")                                            # a lens is fine there
    c = pt.Camera.from_buffer_copy(cam)
    c.defocus_angle = 1.0
    acc, _ = gs.render(c, 1, 0, 4)
    assert np.isfinite(acc).all()
    # and back: the bits of a scene that never had the setting
    gs.set_projection("panorama")
    pano, _ = gs.render(cam, 1, 0, 4, slots_per_pixel=1)
    gs.set_projection(0)
    back, st = gs.render(cam, 1, 0, 4, slots_per_pixel=1)
    fresh = pt.Scene(ctx)
    cam2 = fresh.build_scene(3, 64, 4)
    ref, st2 = fresh.render(cam2, 1, 0, 4, slots_per_pixel=1)
    np.testing.assert_array_equal(back, ref)
    assert st.segments == st2.segments and not np.array_equal(pano, ref)
    assert h == 64
    gs.close(); fresh.close()


# ---- 8. through the CLI: a panorama written as a float image ----------------------------------------------------------------------------
def test_cli_writes_a_panorama_hdr(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    hdr, png = str(tmp_path / "p.hdr"), str(tmp_path / "p.png")
    r = subprocess.run([exe, "-s", "3", "--width", "64", "--spp", "4", "--projection", "panorama", "--out-hdr", hdr, "--out", png, "--assets", pt.ASSET_DIR],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = pt.load_hdr_rgbf32(hdr)
    assert img.shape == (64, 64, 3)                                              # scene 3's aspect ratio is 1
    assert np.isfinite(img).all() and (img >= 0.0).all()
    # The script's camera stands 800 units in front of the box, at half its height: the rows at the poles look straight up and down past
    # the box into the black environment, so it is the two HALVES that differ: the ceiling and its light above the horizon, the lit floor below.
    upper, lower = img[: 32], img[32:]
    assert upper.sum() > 0.0 and lower.sum() > 0.0
    assert not np.array_equal(upper, lower[::-1])
    assert (img[0] == 0.0).all() and (img[-1] == 0.0).all()
    assert (img[:, : 32] == 0.0).all()                                           # the box is at phi = +90 degrees: columns around 3 W / 4
