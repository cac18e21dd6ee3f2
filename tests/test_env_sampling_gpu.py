"""Environment importance sampling (pt_scene_set_env_sampling) on the GPU.

The sampling rule of include/pt_amd.h is restated in numpy and compared with the device functions K3 calls (pt_env_probe); the
estimator is checked against quadrature on a Lambert floor (no oracle: the reference has no such estimator), against today's
estimator where both must have the same expectation, and bit for bit against today's where it must not act at all."""
import os

import numpy as np
import pytest

from common import MIS_ALBEDO, MIS_CAM, SceneSpec, default_camera, mis_zscores

pytestmark = pytest.mark.gpu


# ---- the rule, restated ------------------------------------------------------------------------------------------------
def texel_values(img):
    """The texel values as tex_image returns them: RGB8 * (1/255), or f32 widened to f64."""
    if img.dtype == np.uint8:
        return (1.0 / 255.0) * img.astype(np.float64)
    return img.astype(np.float64)


def tables(img):
    v = texel_values(img)
    H, W = v.shape[:2]
    lum = 0.2126 * v[..., 0] + 0.7152 * v[..., 1] + 0.0722 * v[..., 2]
    lum = np.where(lum > 0.0, lum, 0.0)
    c = np.cos(np.arange(H + 1) * np.pi / H)
    w = (lum * (c[:-1] - c[1:])[:, None]) * ((2.0 * np.pi) / W)
    P = np.concatenate([np.zeros((H, 1)), np.cumsum(w, axis=1)], axis=1)
    Q = np.concatenate([[0.0], np.cumsum(P[:, W])])
    return dict(lum=lum, c=c, w=w, P=P, Q=Q, Z=Q[H], H=H, W=W)


def sample(t, u):
    """(n, 2) draws -> directions (n, 3), pdfs (n,), texels (j, i)."""
    H, W, Q, P, c, Z = t["H"], t["W"], t["Q"], t["P"], t["c"], t["Z"]
    x = u[:, 0] * Z
    x = np.where(x < Z, x, np.nextafter(Z, 0.0))
    j = np.searchsorted(Q[1:], x, side="right")
    t1 = (x - Q[j]) / (Q[j + 1] - Q[j])
    cos_t = c[j] - t1 * (c[j] - c[j + 1])
    R = P[j, W]
    y = u[:, 1] * R
    y = np.where(y < R, y, np.nextafter(R, 0.0))
    i = np.empty_like(j)
    for row in np.unique(j):
        m = j == row
        i[m] = np.searchsorted(P[row, 1:], y[m], side="right")
    t2 = (y - P[j, i]) / (P[j, i + 1] - P[j, i])
    phi = -np.pi + ((2.0 * np.pi) * (i + t2)) / W
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    d = np.stack([sin_t * np.cos(phi), cos_t, sin_t * np.sin(phi)], axis=1)
    return d, t["lum"][j, i] / Z, j, i


def texel_of(t, d):
    """sample_environment's texel for directions d (acos, atan2, tex_image's clamp and Q6 rule)."""
    H, W = t["H"], t["W"]
    theta = np.arccos(np.clip(d[:, 1], -1.0, 1.0))
    phi = np.arctan2(d[:, 2], d[:, 0])
    u = np.clip((phi + np.pi) / (2.0 * np.pi), 0.0, 1.0)
    v = 1.0 - np.clip(1.0 - theta / np.pi, 0.0, 1.0)
    return np.minimum((v * H).astype(np.int64), H - 1), np.minimum((u * W).astype(np.int64), W - 1)


def floor_expectation(img, albedo):
    """E[radiance] of an upward Lambert floor lit by the map alone, one bounce: albedo * sum_{j<H/2} sum_i L_ij (sin^2 th_{j+1} - sin^2 th_j) / W."""
    v = texel_values(img)
    H, W = v.shape[:2]
    th = np.arange(H + 1) * np.pi / H
    ds = np.sin(th[1:]) ** 2 - np.sin(th[:-1]) ** 2
    return np.asarray(albedo) * (v[: H // 2] * ds[: H // 2, None, None]).sum(axis=(0, 1)) / W


def floor_second_moment(img, albedo, f):
    """E[X^2] per channel of the env-on one-bounce floor estimator, X = albedo L (cos/pi) / ((1-f) cos/pi + f q): Gauss-Legendre in
    theta inside every upper-hemisphere row (q is constant over a texel); env samples below the floor add zero."""
    t = tables(img)
    v = texel_values(img)
    H, W = v.shape[:2]
    q = t["lum"] / t["Z"]
    xg, wg = np.polynomial.legendre.leggauss(12)
    out = np.zeros(3)
    for j in range(H // 2):
        a, b = j * np.pi / H, (j + 1) * np.pi / H
        th = 0.5 * (b - a) * xg + 0.5 * (a + b)
        cp = np.cos(th) / np.pi
        g = (cp ** 2 * np.sin(th))[None, :] / ((1.0 - f) * cp[None, :] + f * q[j][:, None])   # (W, nodes)
        row = (g * wg[None, :]).sum(axis=1) * 0.5 * (b - a) * (2.0 * np.pi / W)               # (W,)
        out += (v[j] ** 2 * row[:, None]).sum(axis=0)
    return np.asarray(albedo) ** 2 * out


def synthetic_maps():
    """16 x 8 maps with an all-black row, one black texel and one bright texel; RGB8 and f32."""
    rng = np.random.default_rng(5)
    rgb8 = rng.integers(20, 200, (8, 16, 3)).astype(np.uint8)
    rgb8[6] = 0
    rgb8[2, 3] = 0
    rgb8[1, 9] = 255
    f32 = (rng.random((8, 16, 3)) * 0.4 + 0.1).astype(np.float32)
    f32[6] = 0.0
    f32[2, 3] = 0.0
    f32[1, 9] = (12.0, 10.0, 8.0)
    return rgb8, f32


def grace(pt, float_hdr):
    path = os.path.join(pt.ASSET_DIR, "grace_probe_latlong.hdr")
    return pt.load_hdr_rgbf32(path) if float_hdr else pt.load_hdr_rgb8(path)


def map_scene(pt, ctx, img, floor="diffuse", light=False):
    """mis_scene's camera over a floor of the given kind (no light unless `light`), lit by the map `img`."""
    spec = SceneSpec()
    tex = spec.add("tex_image_rgb8" if img.dtype == np.uint8 else "tex_image_rgbf32", img)
    alb = spec.add("tex_solid_rgb", *MIS_ALBEDO)
    if floor == "diffuse":
        m = spec.add("mat_diffuse", alb, -1)
    elif floor.startswith("metal"):
        m = spec.add("mat_metal", alb, spec.add("tex_solid_f", float(floor[5:] or 0.3)))
    elif floor == "glass":
        m = spec.add("mat_glass", alb, spec.add("tex_solid_f", 0.2), 0.0, 1.5)
    elif floor == "principled":
        m = spec.add("mat_principled", alb, [0.3, 0.4, 0.1, 0.5, 0.1, 1.5, 0.0, 0.2, 0.5, 0.3, 0.6])
    elif floor == "sheen":
        m = spec.add("mat_sheen", MIS_ALBEDO, 0.5)
    elif floor == "clearcoat":
        m = spec.add("mat_clearcoat", 0.7)
    elif floor == "mix":
        m = spec.add("mat_mix", 0.4, spec.add("mat_diffuse", alb, -1), spec.add("mat_metal", alb, spec.add("tex_solid_f", 0.3)))
    spec.add("world_add_object", spec.add("quad", (-4.0, 0.0, -4.0), (0.0, 0.0, 8.0), (8.0, 0.0, 0.0), m))
    if light:
        from common import MIS_EMISSION, MIS_QUAD
        spec.add("world_add_light", spec.add("quad", *MIS_QUAD, spec.add("mat_light", spec.add("tex_solid_rgb", *MIS_EMISSION))))
    spec.add("world_build")
    c = MIS_CAM
    spec.camera = default_camera(width=c["width"], aspect=c["aspect"], spp=1, max_depth=2, vfov=c["vfov"], look_from=c["look_from"],
                                 look_at=c["look_at"], vup=c["vup"], focal_length=c["focal_length"], defocus_angle=0.0, blur_strength=0.5,
                                 env_color=(0.0, 0.0, 0.0), env_is_map=1, env_tex=tex)
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    return gs, cam


def two_sample_z(render_a, render_b, n_batches=16, spp_per_batch=256, seed=3):
    """Per-pixel and image-mean z of two estimators of the same thing (batches of sums / spp)."""
    a = np.stack([render_a(seed, k * spp_per_batch, (k + 1) * spp_per_batch) / spp_per_batch for k in range(n_batches)])
    b = np.stack([render_b(seed + 1, k * spp_per_batch, (k + 1) * spp_per_batch) / spp_per_batch for k in range(n_batches)])
    se2 = lambda x: x.var(axis=0, ddof=1) / n_batches
    z = (a.mean(axis=0) - b.mean(axis=0)) / np.sqrt(se2(a) + se2(b))
    ga, gb = a.mean(axis=(1, 2)), b.mean(axis=(1, 2))
    zg = (ga.mean(axis=0) - gb.mean(axis=0)) / np.sqrt(se2(ga) + se2(gb))
    return z, zg


# ---- 1. the setting ------------------------------------------------------------------------------------------------------
def test_setting_validation(pt, ctx):
    gs = pt.Scene(ctx)
    assert gs.env_sampling() == 0.0
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(pt.PtError):
            gs.set_env_sampling(bad)
        assert gs.env_sampling() == 0.0
    for ok in (0.5, 0.0):
        gs.set_env_sampling(ok)
        assert gs.env_sampling() == ok
    gs.close()


# ---- 2. the device functions against the restated rule -------------------------------------------------------------------
def _maps(pt):
    rgb8, f32 = synthetic_maps()
    return [("rgb8", rgb8), ("f32", f32), ("grace_rgb8", grace(pt, False)), ("grace_f32", grace(pt, True))]


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_probe_matches_numpy_rule(pt, ctx, which):
    name, img = _maps(pt)[which]
    gs, cam = map_scene(pt, ctx, img)
    t = tables(img)
    n = 1 << 20
    u = np.random.default_rng(17 + which).random((n, 2))
    out = gs.env_probe(cam, 0, u)
    d_ref, pdf_ref, j_ref, i_ref = sample(t, u)
    np.testing.assert_allclose(out[:, :3], d_ref, rtol=0.0, atol=1e-12, err_msg=name)
    np.testing.assert_allclose(out[:, 3], pdf_ref, rtol=1e-12, atol=0.0, err_msg=name)
    assert np.abs(np.linalg.norm(out[:, :3], axis=1) - 1.0).max() < 1e-12
    assert (pdf_ref > 0.0).all()                                   # zero-weight rows and texels are never chosen
    # env_pdf at the sampled direction is the sample's pdf (but for texel borders)
    back = gs.env_probe(cam, 1, out[:, :3])
    assert (back != out[:, 3]).sum() <= max(1, int(1e-6 * n)), name
    # env_pdf over the texel centres integrates to one, and agrees with the rule
    H, W = t["H"], t["W"]
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    th, ph = (jj + 0.5) * np.pi / H, -np.pi + (ii + 0.5) * 2.0 * np.pi / W
    dc = np.stack([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)], axis=-1).reshape(-1, 3)
    pc = gs.env_probe(cam, 1, dc).reshape(H, W)
    np.testing.assert_allclose(pc, t["lum"] / t["Z"], rtol=1e-12, atol=0.0)
    omega = (t["c"][:-1] - t["c"][1:])[:, None] * (2.0 * np.pi / W)
    assert abs((pc * omega).sum() - 1.0) < 1e-12
    # texel histogram of the device's samples against w / Z (chi-square; coarse bins for the large maps)
    js, is_ = texel_of(t, out[:, :3])
    bj, bi = (js * min(H, 16)) // H, (is_ * min(W, 32)) // W
    nb = min(H, 16) * min(W, 32)
    p = np.bincount(((np.arange(H)[:, None] * min(H, 16)) // H * min(W, 32) + (np.arange(W)[None, :] * min(W, 32)) // W).reshape(-1),
                    weights=(t["w"] / t["Z"]).reshape(-1), minlength=nb)
    cnt = np.bincount((bj * min(W, 32) + bi).reshape(-1), minlength=nb)
    assert cnt[p == 0.0].sum() == 0
    k = p > 0.0
    chi2 = ((cnt[k] - n * p[k]) ** 2 / (n * p[k])).sum()
    dof = k.sum() - 1
    assert chi2 < dof + 6.0 * np.sqrt(2.0 * dof), (name, chi2, dof)
    gs.close()


def test_probe_refuses_colour_environment(pt, ctx):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 16, 1)
    with pytest.raises(pt.PtError):
        gs.env_probe(cam, 1, np.array([[0.0, 1.0, 0.0]]))
    gs.close()


# ---- 3. off means off ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", [1, 3])
@pytest.mark.parametrize("k", [1, 0])
def test_colour_environment_renders_unchanged(pt, ctx, sid, k):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(sid, 48, 8)
    base, st0 = gs.render(cam, 5, 0, 8, slots_per_pixel=k)
    for f in (0.0, 0.5):
        gs.set_env_sampling(f)
        got, st = gs.render(cam, 5, 0, 8, slots_per_pixel=k)
        assert st.segments == st0.segments and st.samples == st0.samples
        if k == 1:
            np.testing.assert_array_equal(got, base)
        else:   # dynamic mode: the f64 atomics add in any order
            fin = np.isfinite(base)
            assert (np.isfinite(got) == fin).all()
            np.testing.assert_allclose(got[fin], base[fin], rtol=1e-12, atol=0.0)
    gs.close()


@pytest.mark.parametrize("k", [1, 0])
def test_scene_without_env_set_materials_renders_unchanged(pt, ctx, k):
    """Image-lit glass and lights only: the ENV form runs (the map has weight) but no hit is in E."""
    rgb8, _ = synthetic_maps()
    spec = SceneSpec()
    tex = spec.add("tex_image_rgb8", rgb8)
    glass = spec.add("mat_glass", spec.add("tex_solid_rgb", 0.9, 0.9, 0.9), spec.add("tex_solid_f", 0.1), 0.0, 1.5)
    lm = spec.add("mat_light", spec.add("tex_solid_rgb", 4.0, 4.0, 4.0))
    spec.add("world_add_object", spec.add("sphere", 1.0, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), glass))
    spec.add("world_add_object", spec.add("quad", (-4.0, 0.0, -4.0), (0.0, 0.0, 8.0), (8.0, 0.0, 0.0), glass))
    spec.add("world_add_light", spec.add("quad", (-1.0, 3.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), lm))
    spec.add("world_build")
    spec.camera = default_camera(width=40, spp=8, env_is_map=1, env_tex=tex, defocus_angle=0.0)
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    base, st0 = gs.render(cam, 2, 0, 8, slots_per_pixel=k)
    gs.set_env_sampling(0.5)
    got, st = gs.render(cam, 2, 0, 8, slots_per_pixel=k)
    assert st.segments == st0.segments
    if k == 1:
        np.testing.assert_array_equal(got, base)
    else:
        fin = np.isfinite(base)
        np.testing.assert_allclose(got[fin], base[fin], rtol=1e-12, atol=0.0)
    gs.close()


# ---- 4. a Lambert floor under the map, against quadrature -----------------------------------------------------------------
@pytest.mark.parametrize("which", ["f32_patch", "grace_rgb8"])
def test_lambert_floor_matches_quadrature(pt, ctx, which):
    img = synthetic_maps()[1] if which == "f32_patch" else grace(pt, False)
    gs, cam = map_scene(pt, ctx, img)
    e = floor_expectation(img, MIS_ALBEDO)
    h = pt.image_height(cam)
    expected = np.broadcast_to(e, (h, cam.image_width, 3))
    for f in (0.0, 0.5):                                  # today's estimator validates the test, then the mixture
        gs.set_env_sampling(f)
        z, zg, mean = mis_zscores(lambda seed, a, b: gs.render(cam, seed, a, b)[0], expected)
        assert np.isfinite(z).all()
        assert np.abs(zg).max() < 4.0, (f, zg)
        assert (np.abs(z) > 4.0).mean() < 0.01 and 0.85 < z.std() < 1.3, (f, np.abs(z).max(), z.std())
    # the per-sample variance of the mixture is the one its documented pdf predicts: pixel means of a wide frame are i.i.d.
    f, spp = 0.5, 256
    gs.set_env_sampling(f)
    cam.image_width = 64
    acc, _ = gs.render(cam, 9, 0, spp)
    m = acc.reshape(-1, 3) / spp
    var_measured = m.var(axis=0, ddof=1) * spp
    var_predicted = floor_second_moment(img, MIS_ALBEDO, f) - e ** 2
    assert (np.abs(var_measured / var_predicted - 1.0) < 0.15).all(), (var_measured, var_predicted)
    gs.close()


# ---- 5, 6. same expectation as today: lights + environment, and every kind in E --------------------------------------------
@pytest.mark.parametrize("floor, light", [("diffuse", True), ("metal0.3", False), ("metal0.3", True)])
def test_env_on_keeps_expectation(pt, ctx, floor, light):
    img = grace(pt, False)
    gs, cam = map_scene(pt, ctx, img, floor=floor, light=light)

    def render(f):
        def r(seed, a, b):
            gs.set_env_sampling(f)
            return gs.render(cam, seed, a, b)[0]
        return r

    z, zg = two_sample_z(render(0.5), render(0.0))
    gs.close()
    assert np.isfinite(z).all()
    assert (np.abs(z) > 4.0).mean() < 0.01, (np.abs(z).max(), z.std())
    assert np.abs(zg).max() < 4.0, zg


@pytest.mark.parametrize("floor", ["glass", "principled", "sheen", "clearcoat", "mix", "metal0.01"])
def test_kinds_outside_env_set_are_unchanged(pt, ctx, floor):
    gs, cam = map_scene(pt, ctx, grace(pt, False), floor=floor)
    base, st0 = gs.render(cam, 4, 0, 16, slots_per_pixel=1)
    gs.set_env_sampling(0.5)
    got, st = gs.render(cam, 4, 0, 16, slots_per_pixel=1)
    gs.close()
    assert st.segments == st0.segments
    np.testing.assert_array_equal(got, base)


# ---- 7. exact structure in the static mode with the mixture on ------------------------------------------------------------
def test_static_structure_with_env_on(pt, ctx):
    gs = pt.Scene(ctx)
    gs.set_float_hdr(True)
    cam = gs.build_scene(6, 64, 6)
    gs.set_env_sampling(0.5)
    seed, n = 7, 6
    full, _ = gs.render(cam, seed, 0, n, slots_per_pixel=1)
    off = pt.Scene(ctx)
    off.set_float_hdr(True)
    ocam = off.build_scene(6, 64, 6)
    assert not np.array_equal(full, off.render(ocam, seed, 0, n, slots_per_pixel=1)[0])   # the mixture does act here
    off.close()
    parts = np.zeros_like(full)
    for s in range(n):                                   # sample ranges add up, bit for bit
        gs.render(cam, seed, s, s + 1, accum=parts, slots_per_pixel=1)
    np.testing.assert_array_equal(parts, full)
    h, w = full.shape[:2]
    px = np.sort(np.random.default_rng(3).choice(h * w, 700, replace=False)).astype(np.uint32)
    sentinel = np.full_like(full, -3.25)
    lst, _ = gs.render_pixels(cam, seed, px, 0, n, accum=sentinel.copy(), slots_per_pixel=1, overwrite=True)
    mask = np.zeros(h * w, bool)
    mask[px] = True
    mask = mask.reshape(h, w)
    np.testing.assert_array_equal(lst[mask], full[mask])
    np.testing.assert_array_equal(lst[~mask], sentinel[~mask])
    dyn, _ = gs.render(cam, seed, 0, n)
    fin = np.isfinite(full)
    np.testing.assert_allclose(dyn[fin], full[fin], rtol=1e-12, atol=1e-12)
    comm = pt.Comm(ctx, 0, 1)
    multi, _ = gs.render_multi(cam, seed, n, comm, slots_per_pixel=1)
    comm.close()
    np.testing.assert_array_equal(multi, full)
    ada, counts, _ = gs.render_adaptive(cam, seed, 2, n, 0.0, slots_per_pixel=1)
    assert (counts == n).all()
    np.testing.assert_allclose(ada[fin], full[fin], rtol=1e-12, atol=1e-12)
    gs.close()


# ---- 8. the noise it removes on the headline scene with float HDR ---------------------------------------------------------
def rel_mse_trimmed(x, ref):
    """mean over pixels of the channel-mean (x - ref)^2 / (ref^2 + 1e-2), without the 0.1 % largest."""
    e = ((x - ref) ** 2 / (ref ** 2 + 1e-2)).mean(axis=2).reshape(-1)
    return np.sort(e)[: int(len(e) * 0.999)].mean()


ENV_RELMSE_RATIO_MAX = 0.4   # env-on / env-off trimmed relMSE at 64 spp, scene 6 float HDR: measured 0.23


def test_scene6_float_hdr_noise_reduction(pt, ctx):
    gs = pt.Scene(ctx)
    gs.set_float_hdr(True)
    cam = gs.build_scene(6, 240, 64)

    def batches(f, seed0):
        gs.set_env_sampling(f)
        return np.stack([gs.render(cam, seed0 + k, 0, 256)[0] / 256 for k in range(16)])

    on_b, off_b = batches(0.5, 100), batches(0.0, 200)
    ref = on_b.mean(axis=0)                                # 4096 spp with the mixture
    gs.set_env_sampling(0.5)
    on = gs.render(cam, 1, 0, 64)[0] / 64
    gs.set_env_sampling(0.0)
    off = gs.render(cam, 1, 0, 64)[0] / 64
    gs.close()
    r_on, r_off = rel_mse_trimmed(on, ref), rel_mse_trimmed(off, ref)
    print(f"scene 6 float HDR, 64 spp: trimmed relMSE env-on {r_on:.4g}, env-off {r_off:.4g}, ratio {r_on / r_off:.4f}")
    assert r_on <= ENV_RELMSE_RATIO_MAX * r_off, (r_on, r_off)
    # the frame means agree within their statistical error (16 x 256 spp each)
    g_on, g_off = on_b.mean(axis=(1, 2)), off_b.mean(axis=(1, 2))
    se = np.sqrt(g_on.var(axis=0, ddof=1) / len(g_on) + g_off.var(axis=0, ddof=1) / len(g_off))
    z = (g_on.mean(axis=0) - g_off.mean(axis=0)) / se
    print(f"scene 6 float HDR frame means: env-on {g_on.mean(axis=0)}, env-off {g_off.mean(axis=0)}, z {z}")
    assert np.abs(z).max() < 4.0, z


# ---- 9. the CLI ----------------------------------------------------------------------------------------------------------
def test_cli_env_sampling(pt, tmp_path):
    import subprocess
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    out = tmp_path / "x.png"
    r = subprocess.run([exe, "-s", "6", "--width", "64", "--spp", "4", "--float-hdr", "--env-sampling", "0.5", "--out", str(out),
                        "--assets", pt.ASSET_DIR], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert out.stat().st_size > 0
    r = subprocess.run([exe, "-s", "6", "--width", "64", "--spp", "4", "--env-sampling", "1", "--out", str(tmp_path / "y.png"),
                        "--assets", pt.ASSET_DIR], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
