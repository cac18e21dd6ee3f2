"""Homogeneous participating media on the GPU (pt_mat_medium; the rule is in include/pt_amd.h): validation, the
device functions against the numpy restatement (tests/medium_rule.py), "off means off", the exact distribution of transmittance,
the white furnace with media, a scalar replay of whole paths, single scattering against quadrature, and the structural identities
(sample ranges, pixel lists, modes, multi, adaptive, AOVs, the CLI)."""
import os
import subprocess

import numpy as np
import pytest

import medium_rule as MR
import refs_numpy as R
import sampler_rule as SR
from common import SceneSpec, default_camera, icosphere, mis_zscores, random_scene, white_furnace_scene

pytestmark = pytest.mark.gpu

GS = (-0.7, 0.0, 0.3, 0.9)


def build(pt, ctx, spec):
    gs = pt.Scene(ctx)
    res = spec.replay(gs)
    return gs, spec.make_camera(pt.Camera, res), res


# ---- 1. validation -------------------------------------------------------------------------------------------------------
def test_validation(pt, ctx):
    gs = pt.Scene(ctx)
    nan, inf = float("nan"), float("inf")
    for bad in [dict(density=0.0), dict(density=-1.0), dict(density=nan), dict(density=inf), dict(albedo=(1.1, 0.5, 0.5)), dict(albedo=(0.5, -0.1, 0.5)),
                dict(albedo=(0.5, 0.5, nan)), dict(albedo=(0.5, inf, 0.5)), dict(g=1.0), dict(g=-1.0), dict(g=1.5), dict(g=nan)]:
        args = dict(density=1.0, albedo=(0.5, 0.5, 0.5), g=0.0)
        args.update(bad)
        with pytest.raises(pt.PtError):
            gs.mat_medium(**args)
    white = gs.mat_diffuse(gs.tex_solid_rgb(1.0, 1.0, 1.0), -1)
    fog = gs.mat_medium(0.5, (1.0, 1.0, 1.0), 0.3)
    assert fog == white + 1                                  # the refused calls created nothing
    with pytest.raises(pt.PtError):
        gs.mat_mix(0.5, white, fog)
    with pytest.raises(pt.PtError):
        gs.mat_mix(0.5, fog, white)
    ball = gs.sphere(1.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), fog)
    for obj in (ball, gs.instance(ball, (0.0, 1.0, 0.0), 0.3, (1.0, 0.0, 0.0)), gs.cuboid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), fog)):
        with pytest.raises(pt.PtError):
            gs.world_add_light(obj)
    assert gs.camera_medium() == -1
    for bad in (white, 99, -2):
        with pytest.raises(pt.PtError):
            gs.set_camera_medium(bad)
        assert gs.camera_medium() == -1
    gs.set_camera_medium(fog)
    assert gs.camera_medium() == fog
    with pytest.raises(pt.PtError):
        gs.set_camera_medium(white)
    assert gs.camera_medium() == fog                         # a refused call leaves the setting
    gs.set_camera_medium(-1)
    assert gs.camera_medium() == -1
    with pytest.raises(pt.PtError):
        gs.medium_probe(white, 1, np.array([0.5]))
    gs.world_add_object(ball)                                # the world holds only what the accepted calls added
    gs.world_build()
    assert gs.prim_count() == 1
    gs.close()


# ---- 2. the device functions against the rule ------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GS)
def test_probe_matches_rule(pt, ctx, g):
    n = 1 << 20
    rng = np.random.default_rng(11)
    gs = pt.Scene(ctx)
    fog = gs.mat_medium(2.5, (1.0, 1.0, 1.0), g)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    axis[:4] = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, -1.0, 0.0)]
    u = rng.random((n, 2))
    u[:2, 0] = [0.0, 1.0 - 2.0 ** -53]
    out = gs.medium_probe(fog, 0, np.concatenate([u, axis], axis=1))
    want = MR.hg_dir(g, u[:, 0], u[:, 1], axis)
    err_dir = np.abs(out[:, :3] - want).max()
    err_len = np.abs(np.linalg.norm(out[:, :3], axis=1) - 1.0).max()
    cos_t = (out[:, :3] * axis).sum(axis=1)
    ph = MR.hg_phase(g, cos_t)
    err_ph = np.abs(out[:, 3] / ph - 1.0).max()
    uu = rng.random(n)
    uu[0] = 0.0
    dist = gs.medium_probe(fog, 1, uu)
    ref = MR.free_flight(uu, 2.5)
    nz = ref != 0.0
    err_ff = np.abs(dist[nz] / ref[nz] - 1.0).max()
    gs.close()
    print(f"g {g}: direction {err_dir:.3g} abs, length {err_len:.3g}, ph {err_ph:.3g} rel, free flight {err_ff:.3g} rel")
    assert err_dir < 1e-12 and err_len < 1e-12 and err_ph < 1e-12
    assert err_ff < 1e-12 and (dist[~nz] == 0.0).all()
    # the histogram of cos_t against the analytic CDF: 64 equal-probability bins
    c = MR.hg_cos(g, u[2:, 0])
    cos_dev = cos_t[2:]
    # (the frame of vec3.rs:23-29 is a half turn about x for axes within 1e-5 of -z, exact only AT -z: there cos_t is off by up to 5e-3,
    # the rule's ph follows dot(dir, w), and nothing else depends on it)
    cap = (axis[2:, 2] < -0.99999) & (axis[2:, 2] > -1.0)
    assert np.abs(cos_dev - c)[~cap].max() < 1e-12 and cap.mean() < 1e-4
    k = 64
    edges = MR.hg_cos(g, np.arange(1, k) / k) if abs(g) >= 1e-3 else np.sort(MR.hg_cos(g, np.arange(1, k) / k))
    counts = np.bincount(np.searchsorted(edges, cos_dev), minlength=k).astype(np.float64)
    cdf = np.concatenate([[0.0], MR.hg_cdf(g, edges), [1.0]])
    expect = np.diff(cdf) * len(cos_dev)
    chi2 = ((counts - expect) ** 2 / expect).sum()
    dof = k - 1
    assert chi2 < dof + 6.0 * np.sqrt(2.0 * dof), (chi2, dof)
    # the sample mean of cos_t against g, with the variance the rule gives: E[cos^2] = (1 + 2 g^2) / 3
    var = (1.0 + 2.0 * g * g) / 3.0 - g * g
    z = (cos_dev.mean() - g) / np.sqrt(var / len(cos_dev))
    assert abs(z) < 5.0, z


# ---- 3. off means off -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["scene1", "scene3", "random"])
def test_unused_medium_changes_nothing(pt, ctx, which):
    def scene(with_medium):
        gs = pt.Scene(ctx)
        if with_medium:
            gs.mat_medium(0.7, (0.9, 0.8, 0.7), 0.4)
        if which == "random":
            spec = random_scene(5)
            cam = spec.make_camera(pt.Camera, spec.replay(gs))
        else:
            cam = gs.build_scene(int(which[-1]), 64, 8)
        if with_medium:
            gs.mat_medium(1.7, (0.5, 0.5, 0.5), -0.2)       # one before, one after everything else: used by nothing
            gs.world_build()
        return gs, cam

    a, cam_a = scene(False)
    b, cam_b = scene(True)
    ra, sa = a.render(cam_a, 3, 0, 8, slots_per_pixel=1)
    rb, sb = b.render(cam_b, 3, 0, 8, slots_per_pixel=1)
    assert sa.segments == sb.segments
    np.testing.assert_array_equal(rb, ra)
    da, _ = a.render(cam_a, 3, 0, 8)
    db, _ = b.render(cam_b, 3, 0, 8)
    fin = np.isfinite(da)
    np.testing.assert_allclose(db[fin], da[fin], rtol=1e-12, atol=1e-12)
    a.close(); b.close()


# ---- 4. transmittance: the exact distribution ------------------------------------------------------------------------------
ENV = (0.7, 0.8, 0.9)


def z_known_variance(img_sum, n, expect_p):
    """Every sample is E with probability p, else 0: z per pixel and channel with the KNOWN variance E^2 p (1 - p) / n."""
    E = np.array(ENV)
    mean = img_sum / n
    var = (E ** 2) * (expect_p * (1.0 - expect_p))[..., None] / n
    with np.errstate(divide="ignore", invalid="ignore"):          # (p = 1 where no boundary is met: the caller masks those pixels)
        return (mean - E * expect_p[..., None]) / np.sqrt(var)


def accept(z, zg):
    assert np.isfinite(z).all()
    print(f"z: std {z.std():.3f}, max |z| {np.abs(z).max():.2f}, share |z| > 4: {(np.abs(z) > 4).mean():.4f}, image mean z {zg}")
    assert np.abs(zg).max() < 4.0, zg
    assert (np.abs(z) > 4.0).mean() < 0.01
    assert 0.85 < z.std() < 1.3, z.std()


def test_transmittance_camera_inside_sphere(pt, ctx):
    Rr, n = 2.0, 4096
    spec = SceneSpec()
    fog = spec.add("mat_medium", 1.0 / Rr, (0.0, 0.0, 0.0), 0.0)
    spec.add("world_add_object", spec.add("sphere", Rr, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), fog))
    spec.add("set_camera_medium", fog)
    spec.add("world_build")
    spec.camera = default_camera(width=48, spp=1, look_from=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, 1.0), focal_length=1.0, defocus_angle=0.0,
                                 env_color=ENV, max_depth=50)
    gs, cam, _ = build(pt, ctx, spec)
    img, _ = gs.render(cam, 5, 0, n)
    gs.close()
    p = np.full(img.shape[:2], np.exp(-1.0))
    z = z_known_variance(img, n, p)
    zg = (img.mean(axis=(0, 1)) / n - np.array(ENV) * np.exp(-1.0)) / np.sqrt(np.array(ENV) ** 2 * np.exp(-1.0) * (1 - np.exp(-1.0)) / (n * p.size))
    accept(z, zg)


@pytest.mark.parametrize("boundary", ["cuboid", "mesh"])
def test_transmittance_through_a_boundary(pt, ctx, boundary):
    density, n, W = 0.9, 4096, 40
    spec = SceneSpec()
    fog = spec.add("mat_medium", density, (0.0, 0.0, 0.0), 0.0)
    if boundary == "cuboid":
        spec.add("world_add_object", spec.add("cuboid", (-0.9, -0.6, -0.5), (0.8, 0.7, 0.6), fog))
    else:
        P, I = icosphere(1)
        mesh = spec.add("mesh", 0.9, P, I, None, None, fog)
        spec.add("world_add_object", spec.add("instance", mesh, (0.3, 0.8, 0.52), 0.7, (0.1, 0.05, 0.0)))
    spec.add("world_build")
    spec.camera = default_camera(width=W, spp=1, look_from=(0.3, 0.4, -4.0), look_at=(0.0, 0.0, 0.0), vfov=35.0, focal_length=1.0,
                                 defocus_angle=0.0, blur_strength=0.0, env_color=ENV, max_depth=50)
    gs, cam, _ = build(pt, ctx, spec)
    img, _ = gs.render(cam, 6, 0, n)
    # the distance the rule makes a path fly inside: from the OFFSET entry point to the exit hit (pt_intersect twice)
    fr = R.camera_frame(W, 1.0, 35.0, (0.3, 0.4, -4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0)
    H = fr["height"]
    rows, cols = np.divmod(np.arange(H * W), W)
    d = fr["pixel00"] + rows[:, None] * fr["dv"] + cols[:, None] * fr["du"] - fr["center"]
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.concatenate([np.broadcast_to(fr["center"], d.shape), d, np.zeros((len(d), 1))], axis=1)
    h1 = gs.intersect(rays)
    entered = h1[:, 0] == 1.0
    gn = h1[:, 9:12]
    o2 = h1[:, 6:9] + 1e-3 * np.sign((d * gn).sum(axis=1))[:, None] * gn
    h2 = gs.intersect(np.concatenate([o2, d, np.zeros((len(d), 1))], axis=1))
    gs.close()
    assert entered.sum() > 200 and (h2[entered, 0] == 1.0).all()          # a closed boundary: what went in comes out
    L = np.where(entered, h2[:, 1], 0.0)
    p = np.exp(-density * L).reshape(H, W)
    m = entered.reshape(H, W)
    np.testing.assert_allclose(img[~m] / n, np.broadcast_to(ENV, img[~m].shape), rtol=1e-12)   # rays that pass by carry E
    z = z_known_variance(img, n, p)[m]
    E = np.array(ENV)
    zg = ((img[m] / n).mean(axis=0) - E * p[m].mean()) / np.sqrt(E ** 2 * (p[m] * (1 - p[m])).sum() / n) * m.sum()
    accept(z, zg)
    # the uncorrected chord (from the entry point itself) is NOT the expectation at this sample count: the offset matters
    chord = np.exp(-density * (L + 1e-3))[entered].mean()
    assert abs(chord / p[m].mean() - 1.0) > 5e-4


# ---- 5. white furnace with media -------------------------------------------------------------------------------------------
def furnace(g, camera_inside, width, aspect=1.0):
    spec = white_furnace_scene(width=width, aspect=aspect)
    spec.calls = [c for c in spec.calls if c[0] != "world_build"]
    fog = spec.add("mat_medium", 2.0 / 2.4, (1.0, 1.0, 1.0), g)               # optical diameter 2 of the sphere below
    spec.add("world_add_object", spec.add("sphere", 1.2, (-1.3, 1.5, 0.3), (-1.3, 1.5, 0.3), fog))   # encloses the white sphere
    fog2 = spec.add("mat_medium", 2.0 / 1.5, (1.0, 1.0, 1.0), g)
    spec.add("world_add_object", spec.add("cuboid", (1.8, 0.3, -1.0), (3.3, 1.8, 0.5), fog2))        # beside the white cuboid
    if camera_inside:
        haze = spec.add("mat_medium", 2.0 / 16.0, (1.0, 1.0, 1.0), g)
        spec.add("world_add_object", spec.add("cuboid", (-8.0, -1.0, -8.0), (8.0, 9.0, 8.0), haze))   # encloses everything, the camera too
        spec.add("set_camera_medium", haze)
    spec.add("world_build")
    # No path may reach the depth bound: one that does shows as a pixel below the colour. The bound has to be this high because of the
    # one way a path gets held up here: a medium vertex closer than K2's t_min = 1e-3 to a white surface, scattering towards it, steps
    # through it (the rule starts the new ray at the vertex, without an offset) into a closed white object, where nothing absorbs and
    # the only way out is the same step — about 1e-4 per bounce in the haze. Seen at 1920x1080: 4 of 16.6 M samples cut at 20000.
    spec.camera["max_depth"] = 200000
    return spec


@pytest.mark.parametrize("g", [0.0, 0.6])
@pytest.mark.parametrize("camera_inside", [False, True])
def test_white_furnace_with_media(pt, ctx, g, camera_inside):
    spec = furnace(g, camera_inside, 96)
    gs, cam, _ = build(pt, ctx, spec)
    E = np.array(spec.camera["env_color"])
    for k in (0, 1):                                       # the dynamic and the static mode
        img, st = gs.render(cam, 2, 0, 16, slots_per_pixel=k)
        np.testing.assert_allclose(img / 16, np.broadcast_to(E, img.shape), rtol=1e-12, err_msg=f"slots_per_pixel={k}")
    gs.close()


def test_white_furnace_with_media_full_hd(pt, ctx):
    spec = furnace(0.6, True, 1920, 16.0 / 9.0)
    gs, cam, _ = build(pt, ctx, spec)
    E = np.array(spec.camera["env_color"])
    img, st = gs.render(cam, 2, 0, 8)                      # a pool larger than the frame's end: compaction and the shading-order output move m
    gs.close()
    print(f"full-HD furnace: {st.segments / st.samples:.2f} segments per sample, {st.compactions} compactions, {st.iterations} iterations")
    assert img.shape[:2] == (1080, 1920) and st.compactions >= 1
    np.testing.assert_allclose(img / 8, np.broadcast_to(E, img.shape), rtol=1e-12)


# ---- 6. replay ---------------------------------------------------------------------------------------------------------------
REPLAY_CAM = dict(width=32, vfov=40.0, look_from=(0.0, 0.4, -5.0), look_at=(0.0, 0.3, 0.0), max_depth=12, blur_strength=0.5)
REPLAY_MEDIA = [("sphere", 1.5, (0.5, 0.25, 0.125), 0.0), ("cuboid", 2.0, (0.25, 0.5, 1.0), 0.6), ("mesh", 1.0, (1.0, 0.125, 0.5), -0.4)]


def replay_scene():
    """Three media — a sphere, a cuboid, an instanced mesh — with albedos that are different powers of two, nothing else."""
    spec, media = SceneSpec(), MR.Media()
    P, I = icosphere(1)
    for kind, density, albedo, g in REPLAY_MEDIA:
        fog = spec.add("mat_medium", density, albedo, g)
        if kind == "sphere":
            spec.add("world_add_object", spec.add("sphere", 0.8, (-1.2, 0.0, 0.0), (-1.2, 0.0, 0.0), fog))
            media.add_sphere((-1.2, 0.0, 0.0), 0.8, density, albedo, g)
        elif kind == "cuboid":
            spec.add("world_add_object", spec.add("cuboid", (0.2, -0.7, -0.6), (1.6, 0.7, 0.6), fog))
            media.add_box((0.2, -0.7, -0.6), (1.6, 0.7, 0.6), density, albedo, g)
        else:
            mesh = spec.add("mesh", 0.7, P, I, None, None, fog)
            spec.add("world_add_object", spec.add("instance", mesh, (0.0, 1.0, 0.0), 0.4, (0.0, 1.6, 0.3)))
            media.add_mesh(0.7, P, I, (0.0, 1.0, 0.0), 0.4, (0.0, 1.6, 0.3), density, albedo, g)
    spec.add("world_build")
    c = REPLAY_CAM
    spec.camera = default_camera(width=c["width"], spp=1, vfov=c["vfov"], look_from=c["look_from"], look_at=c["look_at"], focal_length=1.0,
                                 defocus_angle=0.0, blur_strength=c["blur_strength"], env_color=(1.0, 1.0, 1.0), max_depth=c["max_depth"])
    return spec, media


@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_replay_of_whole_paths(pt, ctx, sampler):
    spec, media = replay_scene()
    gs, cam, _ = build(pt, ctx, spec)
    gs.set_sampler(sampler)
    c = REPLAY_CAM
    fr = R.camera_frame(c["width"], 1.0, c["vfov"], c["look_from"], c["look_at"], (0.0, 1.0, 0.0), 1.0)
    H, W, seed, n_samples = fr["height"], c["width"], 9, 4
    per_sample = [gs.render(cam, seed, s, s + 1, slots_per_pixel=1)[0].reshape(-1, 3) for s in range(n_samples)]
    gs.close()
    hit_any = per_sample[0][:, 0] != 1.0                                     # pixels whose sample 0 met a medium
    rng = np.random.default_rng(4)
    pixels = np.concatenate([np.flatnonzero(hit_any)[:500], rng.choice(H * W, 250, replace=False)])
    bad, scattered, ended = [], 0, 0
    for p in pixels:
        for s in range(n_samples):
            want = MR.replay_path(media, fr, dict(width=W, blur_strength=c["blur_strength"], max_depth=c["max_depth"]), seed, int(p), s,
                                  (1.0, 1.0, 1.0), sobol=sampler == "sobol")
            got = per_sample[s][p]
            scattered += not np.array_equal(want, np.ones(3))
            ended += not want.any()
            if not np.allclose(got, want, rtol=1e-12, atol=0.0):
                bad.append((int(p), s, got, want))
    n = len(pixels) * n_samples
    print(f"{sampler}: {n} (pixel, sample) pairs, {scattered} met a medium, {ended} ended by roulette or the depth bound, {len(bad)} disagree")
    assert n >= 2000 and scattered > 600 and ended > 20
    assert len(bad) <= 1, bad[:5]


# ---- 7. scattering against quadrature ----------------------------------------------------------------------------------------
SC_QUAD = ((-2.0, 1.5, 0.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0))
SC_CAM = dict(width=12, vfov=30.0, look_from=(0.0, 0.0, -0.5), look_at=(0.0, 0.0, 1.0))
SC_EMISSION, SC_ALBEDO, SC_DENSITY = (6.0, 5.0, 4.0), (0.9, 0.7, 0.5), 0.5


def scatter_scene(pt, ctx, g, in_lights_list):
    spec = SceneSpec()
    fog = spec.add("mat_medium", SC_DENSITY, SC_ALBEDO, g)
    lm = spec.add("mat_light", spec.add("tex_solid_rgb", *SC_EMISSION))
    spec.add("world_add_light" if in_lights_list else "world_add_object", spec.add("quad", *SC_QUAD, lm))
    spec.add("set_camera_medium", fog)
    spec.add("world_build")
    c = SC_CAM
    spec.camera = default_camera(width=c["width"], spp=1, vfov=c["vfov"], look_from=c["look_from"], look_at=c["look_at"], focal_length=1.0,
                                 defocus_angle=0.0, blur_strength=0.0, env_color=(0.0, 0.0, 0.0), max_depth=2)
    return build(pt, ctx, spec)[:2]


@pytest.mark.parametrize("g", [0.0, 0.6])
def test_single_scattering_matches_quadrature(pt, ctx, g):
    """max_depth = 2: radiance = direct transmittance + single scattering. No camera ray of this frame meets the quad (it hangs
    above the view, edge-on), so the direct term is zero here — item 4's tests pin it — and the expectation is the single-scattering
    integral alone, which pins the phase function's normalisation and the MIS weights."""
    c = SC_CAM
    fr = R.camera_frame(c["width"], 1.0, c["vfov"], c["look_from"], c["look_at"], (0.0, 1.0, 0.0), 1.0)
    H, W = fr["height"], c["width"]
    rows, cols = np.divmod(np.arange(H * W), W)
    d = fr["pixel00"] + rows[:, None] * fr["dv"] + cols[:, None] * fr["du"] - fr["center"]
    d /= np.linalg.norm(d, axis=1)[:, None]
    o = np.broadcast_to(fr["center"], d.shape)
    S = MR.single_scatter_quad(o, d, SC_DENSITY, g, SC_QUAD, 48, 40)
    S2 = MR.single_scatter_quad(o, d, SC_DENSITY, g, SC_QUAD, 96, 80)        # (the nearest ray passes 0.4 under the 4 x 4 quad: 2e-5 apart)
    expected = (S2[:, None] * np.array(SC_ALBEDO) * np.array(SC_EMISSION)).reshape(H, W, 3)
    results = {}
    for name, in_list in (("lights list", True), ("plain object", False)):
        gs, cam = scatter_scene(pt, ctx, g, in_list)
        if name == "lights list":
            hits = gs.intersect(np.concatenate([o, d, np.zeros((len(d), 1))], axis=1))
            assert (hits[:, 0] == 0.0).all()                                 # no direct term in this frame
        batches = np.stack([gs.render(cam, 3 + in_list, k * 256, (k + 1) * 256)[0] / 256 for k in range(16)])
        gs.close()
        results[name] = batches
        mean, sem = batches.mean(axis=0), batches.std(axis=0, ddof=1) / 4.0
        z = (mean - expected) / sem
        g_ = batches.mean(axis=(1, 2))
        zg = (g_.mean(axis=0) - expected.mean(axis=(0, 1))) / (g_.std(axis=0, ddof=1) / 4.0)
        quad_err = np.abs(S / S2 - 1.0).max()
        print(f"g {g}, {name}: quadrature changes by {quad_err:.3g} on doubling the nodes; smallest relative standard error {np.min(sem / expected):.3g}")
        assert quad_err * 100.0 < np.min(sem / expected)                     # the quadrature's error is two orders below the noise
        accept(z, zg)
    a, b = results["lights list"], results["plain object"]
    se2 = lambda x: x.var(axis=0, ddof=1) / len(x)
    z = (a.mean(axis=0) - b.mean(axis=0)) / np.sqrt(se2(a) + se2(b))
    ga, gb = a.mean(axis=(1, 2)), b.mean(axis=(1, 2))
    zg = (ga.mean(axis=0) - gb.mean(axis=0)) / np.sqrt(se2(ga) + se2(gb))
    assert np.isfinite(z).all() and (np.abs(z) > 4.0).mean() < 0.01 and np.abs(zg).max() < 4.0, (np.abs(z).max(), zg)


# ---- 8. structure ------------------------------------------------------------------------------------------------------------
def fog_cornell(pt, ctx):
    """Scene 3 inside a box of fog with the camera in it, plus a ball of denser smoke: lights, instances, every branch of the rule."""
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 64, 6)
    fog = gs.mat_medium(0.001, (0.9, 0.9, 0.9), 0.5)
    gs.world_add_object(gs.cuboid((-60.0, -60.0, -900.0), (620.0, 620.0, 620.0), fog))
    smoke = gs.mat_medium(0.01, (0.6, 0.7, 0.8), -0.3)
    gs.world_add_object(gs.sphere(80.0, (380.0, 400.0, 200.0), (380.0, 400.0, 200.0), smoke))
    gs.set_camera_medium(fog)
    gs.world_build()
    return gs, cam


def test_structure_with_media(pt, ctx):
    gs, cam = fog_cornell(pt, ctx)
    seed, n = 7, 6
    full, st = gs.render(cam, seed, 0, n, slots_per_pixel=1)
    plain = pt.Scene(ctx)
    pcam = plain.build_scene(3, 64, 6)
    base, st0 = plain.render(pcam, seed, 0, n, slots_per_pixel=1)
    plain.close()
    assert not np.array_equal(full, base) and st.segments > st0.segments      # the media do act here
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
    fin = np.isfinite(full)
    dyn, _ = gs.render(cam, seed, 0, n)
    np.testing.assert_allclose(dyn[fin], full[fin], rtol=1e-12, atol=1e-12)
    dlst, _ = gs.render_pixels(cam, seed, px, 0, n)
    np.testing.assert_allclose(dlst[mask & fin.all(axis=2)], full[mask & fin.all(axis=2)], rtol=1e-12, atol=1e-12)
    comm = pt.Comm(ctx, 0, 1)
    multi, _ = gs.render_multi(cam, seed, n, comm, slots_per_pixel=1)
    comm.close()
    np.testing.assert_array_equal(multi, full)
    ada, counts, _ = gs.render_adaptive(cam, seed, 2, n, 0.0, slots_per_pixel=1)
    assert (counts == n).all()
    np.testing.assert_allclose(ada[fin], full[fin], rtol=1e-12, atol=1e-12)
    gs.set_sampler("sobol")                              # the Sobol forms: the same identities
    qfull, _ = gs.render(cam, seed, 0, n, slots_per_pixel=1)
    assert not np.array_equal(qfull, full)
    qdyn, _ = gs.render(cam, seed, 0, n)
    qfin = np.isfinite(qfull)
    np.testing.assert_allclose(qdyn[qfin], qfull[qfin], rtol=1e-12, atol=1e-12)
    gs.close()


def test_env_sampling_with_media_is_refused(pt, ctx):
    gs = pt.Scene(ctx)
    gs.set_float_hdr(True)
    cam = gs.build_scene(6, 32, 2)
    gs.set_env_sampling(0.5)
    gs.render(cam, 1, 0, 1)                                  # fine without media
    fog = gs.mat_medium(0.1, (1.0, 1.0, 1.0), 0.0)
    gs.world_build()
    gs.render(cam, 1, 0, 1)                                  # a medium nothing uses is not in effect
    gs.set_camera_medium(fog)
    with pytest.raises(pt.PtError, match="participating media"):
        gs.render(cam, 1, 0, 1)
    gs.set_env_sampling(0.0)
    gs.render(cam, 1, 0, 1)
    gs.close()


def test_aovs_see_a_boundary_as_a_first_hit(pt, ctx):
    spec = SceneSpec()
    fog = spec.add("mat_medium", 0.5, (0.3, 0.4, 0.5), 0.2)
    spec.add("world_add_object", spec.add("quad", (-50.0, -50.0, 3.0), (100.0, 0.0, 0.0), (0.0, 100.0, 0.0), fog))   # fills the frame
    spec.add("world_build")
    spec.camera = default_camera(width=32, spp=1, look_from=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, 1.0), focal_length=1.0, defocus_angle=0.0,
                                 blur_strength=0.0)
    gs, cam, _ = build(pt, ctx, spec)
    aov = gs.render_aovs(cam, 1, 0, 4)
    fr = R.camera_frame(32, 1.0, 50.0, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 1.0)
    rows, cols = np.divmod(np.arange(32 * fr["height"]), 32)
    d = fr["pixel00"] + rows[:, None] * fr["dv"] + cols[:, None] * fr["du"] - fr["center"]
    d /= np.linalg.norm(d, axis=1)[:, None]
    hits = gs.intersect(np.concatenate([np.zeros_like(d), d, np.zeros((len(d), 1))], axis=1))
    gs.close()
    assert (hits[:, 0] == 1.0).all()                         # pt_intersect reports the boundary as an ordinary hit
    np.testing.assert_array_equal(aov[..., 0:3], 4.0)
    np.testing.assert_array_equal(aov[..., 7], 4.0)
    np.testing.assert_allclose(aov[..., 6].reshape(-1) / 4.0, 3.0 / d[:, 2], rtol=1e-12)
    np.testing.assert_allclose(aov[..., 6].reshape(-1) / 4.0, hits[:, 1], rtol=1e-12)


def test_cli_fog(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    out = tmp_path / "fog.png"
    r = subprocess.run([exe, "-s", "3", "--width", "64", "--spp", "8", "--fog", "0.002,0.9,0.9,0.9,0.4", "--out", str(out), "--assets", pt.ASSET_DIR],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    fogged = pt.decode_image_rgb8(str(out)).astype(np.float64)
    clear = tmp_path / "clear.png"
    r = subprocess.run([exe, "-s", "3", "--width", "64", "--spp", "8", "--out", str(clear), "--assets", pt.ASSET_DIR], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.abs(fogged - pt.decode_image_rgb8(str(clear)).astype(np.float64)).mean() > 1.0     # the fog is in the picture
    r = subprocess.run([exe, "-s", "6", "--width", "32", "--spp", "2", "--fog", "0.1", "--sampler", "sobol", "--out", str(tmp_path / "s.png"), "--assets",
                        pt.ASSET_DIR], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
