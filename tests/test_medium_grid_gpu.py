"""Grid-density participating media on the GPU (pt_mat_medium_grid; the rule is in include/pt_amd.h), section by section
as tests/test_medium_gpu.py: validation, the device functions against the numpy restatement (tests/medium_grid_rule.py), "off means
off", the exact distribution of transmittance, the white furnace, a scalar replay of whole paths, single scattering against
quadrature, a constant grid against the homogeneous medium, the structural identities and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import medium_grid_rule as GR
import refs_numpy as R
from common import SceneSpec, default_camera, white_furnace_scene
from test_medium_gpu import ENV, accept, z_known_variance

pytestmark = pytest.mark.gpu

BOX = ((-0.9, -0.6, -0.5), (0.8, 0.7, 0.6))                              # §12's cuboid


def random_values(seed, shape=(7, 5, 6), zeros=0.3):
    """(nz, ny, nx) float32 in [0, 1) with a share of empty cells."""
    rng = np.random.default_rng(seed)
    v = rng.random(shape).astype(np.float32)
    v[rng.random(shape) < zeros] = 0.0
    return v


def build(pt, ctx, spec):
    gs = pt.Scene(ctx)
    res = spec.replay(gs)
    return gs, spec.make_camera(pt.Camera, res), res


def pixel_rays(fr, W):
    H = fr["height"]
    rows, cols = np.divmod(np.arange(H * W), W)
    d = fr["pixel00"] + rows[:, None] * fr["dv"] + cols[:, None] * fr["du"] - fr["center"]
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.broadcast_to(fr["center"], d.shape).copy(), d


# ---- 1. validation -------------------------------------------------------------------------------------------------------
def test_validation(pt, ctx):
    gs = pt.Scene(ctx)
    nan, inf = float("nan"), float("inf")
    v = random_values(1)
    good = dict(scale=1.0, albedo=(0.5, 0.5, 0.5), g=0.0, values=v, box_lo=BOX[0], box_hi=BOX[1])
    neg, bad_nan, bad_inf = v.copy(), v.copy(), v.copy()
    neg[3, 2, 1], bad_nan[0, 0, 0], bad_inf[6, 4, 5] = -1e-6, nan, inf
    diag = float(np.linalg.norm(np.array(BOX[1]) - np.array(BOX[0])))
    too_thick = 4096.0 / (float(v.max()) * diag) * (1.0 + 1e-9)
    refusals = [dict(scale=0.0), dict(scale=-1.0), dict(scale=nan), dict(scale=inf), dict(values=neg), dict(values=bad_nan), dict(values=bad_inf),
                dict(values=np.zeros_like(v)), dict(values=v[:1]), dict(values=v[:, :1]), dict(values=v[:, :, :1]),
                dict(box_lo=(0.8, -0.6, -0.5)), dict(box_lo=(-0.9, 0.9, -0.5)), dict(box_hi=(0.8, 0.7, -0.5)), dict(box_lo=(nan, -0.6, -0.5)),
                dict(box_hi=(0.8, inf, 0.6)), dict(box_lo=(-inf, -0.6, -0.5)),
                dict(albedo=(1.1, 0.5, 0.5)), dict(albedo=(0.5, -0.1, 0.5)), dict(albedo=(0.5, 0.5, nan)), dict(g=1.0), dict(g=-1.0), dict(g=nan),
                dict(scale=too_thick), dict(scale=1e6)]
    for bad in refusals:
        args = dict(good)
        args.update(bad)
        with pytest.raises(pt.PtError):
            gs.mat_medium_grid(**args)
    lo, hi = (C.c_double * 3)(*BOX[0]), (C.c_double * 3)(*BOX[1])      # nx * ny * nz = 2^28 + 2^20: refused before a value is read
    assert pt.lib.pt_mat_medium_grid(gs.handle, 1.0, 0.5, 0.5, 0.5, 0.0, 1 << 10, 1 << 10, (1 << 8) + 1, v.ctypes.data, lo, hi) == -1
    white = gs.mat_diffuse(gs.tex_solid_rgb(1.0, 1.0, 1.0), -1)
    smoke = gs.mat_medium_grid(**dict(good, scale=too_thick / (1.0 + 1e-9) * (1.0 - 1e-9)))   # just inside the design limit
    assert smoke == white + 1                                           # the refused calls created nothing
    fog = gs.mat_medium(0.5, (1.0, 1.0, 1.0), 0.3)
    assert fog == smoke + 1
    for pair in ((white, smoke), (smoke, white)):
        with pytest.raises(pt.PtError):
            gs.mat_mix(0.5, *pair)
    ball = gs.sphere(1.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), smoke)
    for obj in (ball, gs.instance(ball, (0.0, 1.0, 0.0), 0.3, (1.0, 0.0, 0.0)), gs.cuboid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), smoke)):
        with pytest.raises(pt.PtError):
            gs.world_add_light(obj)
    gs.set_camera_medium(smoke)
    assert gs.camera_medium() == smoke
    gs.set_camera_medium(-1)
    for which in (2, 3):                                                # the grid probes refuse a medium without a grid, and a non-medium
        with pytest.raises(pt.PtError):
            gs.medium_probe(fog, which, np.zeros((1, 3 if which == 2 else 7)))
        with pytest.raises(pt.PtError):
            gs.medium_probe(white, which, np.zeros((1, 3 if which == 2 else 7)))
    with pytest.raises(pt.PtError):
        gs.medium_probe(smoke, 3, np.array([[0.0, 0.0, -4.0, 0.0, 0.0, 2.0, np.inf]]))      # a direction longer than 1
    assert gs.medium_probe(smoke, 1, np.array([0.0]))[0] == 0.0         # the existing probes stay
    gs.world_add_object(ball)
    gs.world_build()
    assert gs.prim_count() == 1
    gs.close()


# ---- 2. the device functions against the rule ------------------------------------------------------------------------------
def test_probe_density_matches_rule(pt, ctx):
    n = 1 << 20
    rng = np.random.default_rng(11)
    v = random_values(2)
    lo, hi = np.array(BOX[0]), np.array(BOX[1])
    g = GR.Grid(2.5, v, lo, hi)
    gs = pt.Scene(ctx)
    smoke = gs.mat_medium_grid(2.5, (1.0, 1.0, 1.0), 0.0, v, lo, hi)
    x = lo + (hi - lo) * (rng.random((n, 3)) * 1.5 - 0.25)              # inside and outside
    q = n // 8                                                           # on the faces, edges and corners: coordinates pinned to lo / hi
    pin = rng.integers(0, 3, size=(q, 3))
    x[:q] = np.where(pin == 0, lo, np.where(pin == 1, hi, np.clip(x[:q], lo, hi)))
    k, j, i = np.meshgrid(np.arange(7), np.arange(5), np.arange(6), indexing="ij")
    centres = lo + (np.stack([i, j, k], axis=-1).reshape(-1, 3) + 0.5) / g.cells
    x[q:q + len(centres)] = centres
    x[q + len(centres)] = [np.nan, 0.0, 0.0]
    out = gs.medium_probe(smoke, 2, x)
    gs.close()
    want = g.sigma(x)
    inside = ((x >= lo) & (x <= hi)).all(axis=1)
    assert inside[:q].all() and 0.2 < inside[q:].mean() < 0.5
    assert (out[~inside] == 0.0).all() and (want[~inside] == 0.0).all()
    nz = want != 0.0
    err = np.abs(out[nz] / want[nz] - 1.0).max()
    print(f"sigma: {nz.sum()} non-zero points, max relative error {err:.3g}; largest sigma / mu {out.max() / g.mu:.6f}")
    assert err < 1e-12 and (out[~nz] == 0.0).all()
    assert (out <= g.mu).all()


def test_probe_tracking_matches_rule(pt, ctx):
    n = 1 << 16
    rng = np.random.default_rng(12)
    v = random_values(3)
    lo, hi = np.array(BOX[0]), np.array(BOX[1])
    g = GR.Grid(6.0, v, lo, hi)
    gs = pt.Scene(ctx)
    smoke = gs.mat_medium_grid(6.0, (1.0, 1.0, 1.0), 0.0, v, lo, hi)
    o = np.array([0.3, 0.4, -4.0]) + 0.3 * rng.normal(size=(n, 3))
    o[n // 2:] = lo + (hi - lo) * rng.random((n - n // 2, 3))          # half of the rays start inside the box
    d = rng.normal(size=(n, 3))
    d[:n // 2] = -o[:n // 2] + 0.5 * rng.normal(size=(n // 2, 3))       # the others aim at it, some miss
    d /= np.linalg.norm(d, axis=1)[:, None]
    d = np.nextafter(d, 0.0)                                             # |d| <= 1 to the last bit
    d[:6] = [(0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 0.6, 0.8), (0.6, 0.0, 0.8)]   # axes with dir_a == 0
    o[:3] = [(0.0, 0.0, -3.0), (0.0, -3.0, 0.0), (-3.0, 0.0, 0.9)]
    t = np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.0, 5.0, n))
    out = gs.medium_probe(smoke, 3, np.concatenate([o, d, t[:, None]], axis=1))
    gs.close()
    collided, s, draws = g.track_many(o, d, t, GR.probe_units)
    flag_bad = (out[:, 0] != collided) | (out[:, 2] != draws)
    same = ~flag_bad & collided
    err = np.abs(out[same, 1] / s[same] - 1.0).max()
    print(f"tracking: {collided.mean():.3f} collide, {(draws == 0).mean():.3f} miss the box, mean draws {draws.mean():.2f}, max {draws.max()}; "
          f"{flag_bad.sum()} rows disagree in flag or count, s max relative error {err:.3g}")
    assert 0.2 < collided.mean() < 0.8 and 0.05 < (draws == 0).mean() < 0.6
    assert flag_bad.sum() <= 1, np.flatnonzero(flag_bad)[:5]
    assert err < 1e-12 and (out[~flag_bad & ~collided, 1] == 0.0).all()
    assert not collided[2] and draws[2] == 0                           # (row 2 passes beside the box along an axis)


# ---- 3. off means off -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["scene1", "scene3", "fog_cornell"])
def test_unused_grid_medium_changes_nothing(pt, ctx, which):
    def scene(with_grid):
        gs = pt.Scene(ctx)
        if with_grid:
            gs.mat_medium_grid(0.7, (0.9, 0.8, 0.7), 0.4, random_values(4), (-60.0, -60.0, -900.0), (620.0, 620.0, 620.0))
        cam = gs.build_scene(3 if which == "fog_cornell" else int(which[-1]), 64, 8)
        if which == "fog_cornell":                                       # homogeneous media in effect: the §12 forms and their bits
            fog = gs.mat_medium(0.001, (0.9, 0.9, 0.9), 0.5)
            gs.world_add_object(gs.cuboid((-60.0, -60.0, -900.0), (620.0, 620.0, 620.0), fog))
            smoke = gs.mat_medium(0.01, (0.6, 0.7, 0.8), -0.3)
            gs.world_add_object(gs.sphere(80.0, (380.0, 400.0, 200.0), (380.0, 400.0, 200.0), smoke))
            gs.set_camera_medium(fog)
        if with_grid:
            gs.mat_medium_grid(0.002, (0.5, 0.5, 0.5), -0.2, random_values(5), (0.0, 0.0, 0.0), (555.0, 555.0, 555.0))   # one before, one after: used by nothing
        if with_grid or which == "fog_cornell":
            gs.world_build()
        return gs, cam

    a, cam_a = scene(False)
    b, cam_b = scene(True)
    ra, sa = a.render(cam_a, 3, 0, 8, slots_per_pixel=1)
    rb, sb = b.render(cam_b, 3, 0, 8, slots_per_pixel=1)
    assert sa.segments == sb.segments and sa.shade_variant == sb.shade_variant
    np.testing.assert_array_equal(rb, ra)                                # equal bits: the render took the forms it takes without grid media
    b.set_sampler("sobol"); a.set_sampler("sobol")
    qa, _ = a.render(cam_a, 3, 0, 8, slots_per_pixel=1)
    qb, _ = b.render(cam_b, 3, 0, 8, slots_per_pixel=1)
    np.testing.assert_array_equal(qb, qa)
    b.set_sampler("independent"); a.set_sampler("independent")
    da, _ = a.render(cam_a, 3, 0, 8)
    db, _ = b.render(cam_b, 3, 0, 8)
    fin = np.isfinite(da)
    np.testing.assert_allclose(db[fin], da[fin], rtol=1e-12, atol=1e-12)
    a.close(); b.close()


# ---- 4. transmittance: the exact distribution ------------------------------------------------------------------------------
T_FROM, T_W, T_N = (0.3, 0.4, -4.0), 40, 4096


@pytest.mark.parametrize("setup", ["unbounded", "cuboid"])
def test_transmittance_is_exp_minus_tau(pt, ctx, setup):
    """Albedo 0, environment E: every sample is E with probability exp(-tau) and 0 otherwise. (a) an unbounded grid as the camera
    medium: tau from the box clip alone; (b) a cuboid boundary equal to the box: tau from the OFFSET entry point to the exit hit.
    On the rule alone (numpy tracking, this grid, 40 x 40 rays): std of z 0.97, max |z| 3.2, image z -1.1, 1.5 tentative collisions
    per sample."""
    v = random_values(1)
    g = GR.Grid(2.5, v, BOX[0], BOX[1])
    spec = SceneSpec()
    smoke = spec.add("mat_medium_grid", 2.5, (0.0, 0.0, 0.0), 0.0, v, BOX[0], BOX[1])
    if setup == "cuboid":
        spec.add("world_add_object", spec.add("cuboid", BOX[0], BOX[1], smoke))
    else:
        spec.add("set_camera_medium", smoke)
        # (a world cannot be empty: a small dark ball behind the camera, which no camera ray meets)
        spec.add("world_add_object", spec.add("sphere", 0.1, (0.3, 0.4, -9.0), (0.3, 0.4, -9.0), spec.add("mat_diffuse", spec.add("tex_solid_rgb", 0.0, 0.0, 0.0), -1)))
    spec.add("world_build")
    spec.camera = default_camera(width=T_W, spp=1, look_from=T_FROM, look_at=(0.0, 0.0, 0.0), vfov=35.0, focal_length=1.0, defocus_angle=0.0,
                                 blur_strength=0.0, env_color=ENV, max_depth=50)
    gs, cam, _ = build(pt, ctx, spec)
    img, st = gs.render(cam, 6, 0, T_N)
    fr = R.camera_frame(T_W, 1.0, 35.0, T_FROM, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0)
    H = fr["height"]
    o, d = pixel_rays(fr, T_W)
    if setup == "cuboid":
        h1 = gs.intersect(np.concatenate([o, d, np.zeros((len(d), 1))], axis=1))
        entered = h1[:, 0] == 1.0
        gn = h1[:, 9:12]
        o2 = h1[:, 6:9] + 1e-3 * np.sign((d * gn).sum(axis=1))[:, None] * gn
        h2 = gs.intersect(np.concatenate([o2, d, np.zeros((len(d), 1))], axis=1))
        assert entered.sum() > 200 and (h2[entered, 0] == 1.0).all()
        tau = np.array([g.tau(o2[i], d[i], h2[i, 1]) if entered[i] else 0.0 for i in range(len(d))])
    else:
        assert (gs.intersect(np.concatenate([o, d, np.zeros((len(d), 1))], axis=1))[:, 0] == 0.0).all()
        tau = np.array([g.tau(o[i], d[i]) for i in range(len(d))])
    gs.close()
    p = np.exp(-tau).reshape(H, T_W)
    m = (tau > 0.0).reshape(H, T_W)
    print(f"{setup}: {m.sum()} of {m.size} rays meet the medium, tau up to {tau.max():.2f}, {st.segments / st.samples:.2f} segments per sample")
    assert m.sum() > 200
    # tau = 0: every sample is E exactly, so the pixel is the sum of T_N equal addends, whatever their order
    np.testing.assert_array_equal(img[~m], np.broadcast_to(np.cumsum(np.broadcast_to(ENV, (T_N, 3)), axis=0)[-1], img[~m].shape))
    z = z_known_variance(img, T_N, p)[m]
    E = np.array(ENV)
    zg = ((img[m] / T_N).mean(axis=0) - E * p[m].mean()) / np.sqrt(E ** 2 * (p[m] * (1 - p[m])).sum() / T_N) * m.sum()
    accept(z, zg)


# ---- 5. white furnace with grid media --------------------------------------------------------------------------------------
def furnace(g, width, aspect=1.0):
    """Three grid media of albedo 1: one inside a sphere boundary around the white sphere, one in a cuboid beside the white cuboid,
    one as an unbounded camera medium over the whole scene."""
    spec = white_furnace_scene(width=width, aspect=aspect)
    spec.calls = [c for c in spec.calls if c[0] != "world_build"]
    a = spec.add("mat_medium_grid", 2.0 / 2.4, (1.0, 1.0, 1.0), g, random_values(7, (5, 6, 4)) * 2.0, (-2.6, 0.2, -1.0), (0.0, 2.8, 1.6))
    spec.add("world_add_object", spec.add("sphere", 1.2, (-1.3, 1.5, 0.3), (-1.3, 1.5, 0.3), a))
    b = spec.add("mat_medium_grid", 2.0 / 1.5, (1.0, 1.0, 1.0), g, random_values(8, (3, 8, 5)) * 2.0, (1.8, 0.3, -1.0), (3.3, 1.8, 0.5))
    spec.add("world_add_object", spec.add("cuboid", (1.8, 0.3, -1.0), (3.3, 1.8, 0.5), b))
    haze = spec.add("mat_medium_grid", 2.0 / 12.0, (1.0, 1.0, 1.0), g, random_values(9, (9, 4, 8)) * 2.0, (-7.0, -0.5, -6.5), (7.0, 6.0, 7.0))   # the camera is inside the box
    spec.add("set_camera_medium", haze)
    spec.add("world_build")
    spec.camera["max_depth"] = 200000                                    # (as in §12's furnace: no path may reach the depth bound)
    return spec


@pytest.mark.parametrize("g", [0.0, 0.6])
def test_white_furnace_with_grid_media(pt, ctx, g):
    spec = furnace(g, 96)
    gs, cam, _ = build(pt, ctx, spec)
    E = np.array(spec.camera["env_color"])
    for k in (0, 1):                                                     # the dynamic and the static mode
        img, st = gs.render(cam, 2, 0, 16, slots_per_pixel=k)
        np.testing.assert_allclose(img / 16, np.broadcast_to(E, img.shape), rtol=1e-12, err_msg=f"slots_per_pixel={k}")
    plain = pt.Scene(ctx)
    pspec = white_furnace_scene(width=96)
    pcam = pspec.make_camera(pt.Camera, pspec.replay(plain))
    _, st0 = plain.render(pcam, 2, 0, 16, slots_per_pixel=1)
    plain.close(); gs.close()
    assert st.segments > st0.segments                                   # the media do scatter here


def test_white_furnace_with_grid_media_full_hd(pt, ctx):
    spec = furnace(0.6, 1920, 16.0 / 9.0)
    gs, cam, _ = build(pt, ctx, spec)
    E = np.array(spec.camera["env_color"])
    img, st = gs.render(cam, 2, 0, 8)
    gs.close()
    print(f"full-HD furnace: {st.segments / st.samples:.2f} segments per sample, {st.compactions} compactions, {st.iterations} iterations")
    assert img.shape[:2] == (1080, 1920) and st.compactions >= 1
    np.testing.assert_allclose(img / 8, np.broadcast_to(E, img.shape), rtol=1e-12)


# ---- 6. replay ---------------------------------------------------------------------------------------------------------------
REPLAY_CAM = dict(width=32, vfov=40.0, look_from=(0.0, 0.4, -5.0), look_at=(0.0, 0.3, 0.0), max_depth=12, blur_strength=0.5)
REPLAY_BOX = ((0.2, -0.7, -0.6), (1.6, 0.7, 0.6))
REPLAY_HAZE_BOX = ((-2.4, -1.1, -2.6), (2.2, 1.9, -1.2))                 # a slab between the camera and the objects
REPLAY_GRID = (3.0, (0.25, 0.5, 1.0), 0.6)                               # scale, albedo (powers of two), g
REPLAY_HAZE = (1.2, (0.5, 1.0, 0.25), -0.3)
REPLAY_BALL = (1.5, (0.5, 0.25, 0.125), 0.0)


def replay_media():
    """The rule's view of the replay scene: (Media, the camera medium's index)."""
    media = GR.Media()
    media.add_box(*REPLAY_BOX, GR.Grid(REPLAY_GRID[0], random_values(21, (5, 6, 7)), *REPLAY_BOX), *REPLAY_GRID[1:])
    media.add_sphere((-1.2, 0.0, 0.0), 0.8, *REPLAY_BALL)
    cm = media.add_unbounded(GR.Grid(REPLAY_HAZE[0], random_values(22, (4, 7, 9)), *REPLAY_HAZE_BOX), *REPLAY_HAZE[1:])
    return media, cm


def replay_scene():
    spec = SceneSpec()
    smoke = spec.add("mat_medium_grid", REPLAY_GRID[0], REPLAY_GRID[1], REPLAY_GRID[2], random_values(21, (5, 6, 7)), *REPLAY_BOX)
    spec.add("world_add_object", spec.add("cuboid", *REPLAY_BOX, smoke))
    fog = spec.add("mat_medium", *REPLAY_BALL)
    spec.add("world_add_object", spec.add("sphere", 0.8, (-1.2, 0.0, 0.0), (-1.2, 0.0, 0.0), fog))
    haze = spec.add("mat_medium_grid", REPLAY_HAZE[0], REPLAY_HAZE[1], REPLAY_HAZE[2], random_values(22, (4, 7, 9)), *REPLAY_HAZE_BOX)
    spec.add("set_camera_medium", haze)
    spec.add("world_build")
    c = REPLAY_CAM
    spec.camera = default_camera(width=c["width"], spp=1, vfov=c["vfov"], look_from=c["look_from"], look_at=c["look_at"], focal_length=1.0,
                                 defocus_angle=0.0, blur_strength=c["blur_strength"], env_color=(1.0, 1.0, 1.0), max_depth=c["max_depth"])
    return spec


@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_replay_of_whole_paths(pt, ctx, sampler):
    media, cm = replay_media()
    gs, cam, _ = build(pt, ctx, replay_scene())
    gs.set_sampler(sampler)
    c = REPLAY_CAM
    fr = R.camera_frame(c["width"], 1.0, c["vfov"], c["look_from"], c["look_at"], (0.0, 1.0, 0.0), 1.0)
    H, W, seed, n_samples = fr["height"], c["width"], 9, 4
    per_sample = [gs.render(cam, seed, s, s + 1, slots_per_pixel=1)[0].reshape(-1, 3) for s in range(n_samples)]
    gs.close()
    pixels = np.random.default_rng(4).choice(H * W, 520, replace=False)
    bad, met, ended = [], 0, 0
    for p in pixels:
        for s in range(n_samples):
            want, touched = GR.replay_path(media, fr, dict(width=W, blur_strength=c["blur_strength"], max_depth=c["max_depth"]), seed, int(p), s,
                                           (1.0, 1.0, 1.0), camera_medium=cm, sobol=sampler == "sobol")
            got = per_sample[s][p]
            met += touched
            ended += not want.any()
            if not np.allclose(got, want, rtol=1e-12, atol=0.0):
                bad.append((int(p), s, got, want))
    n = len(pixels) * n_samples
    print(f"{sampler}: {n} (pixel, sample) pairs, {met} met a medium, {ended} ended by roulette or the depth bound, {len(bad)} disagree")
    assert n >= 2000 and met >= 600
    assert len(bad) <= 1, bad[:5]


# ---- 7. single scattering against quadrature ---------------------------------------------------------------------------------
SC_QUAD = ((-2.0, 1.5, 0.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0))
SC_CAM = dict(width=12, vfov=30.0, look_from=(0.0, 0.0, -0.5), look_at=(0.0, 0.0, 1.0))
SC_EMISSION, SC_ALBEDO = (6.0, 5.0, 4.0), (0.9, 0.7, 0.5)
SC_RAMP = dict(scale=0.8, v0=0.25, v1=1.0, n=(4, 3, 7), axis=2, lo=(-3.0, -2.0, 0.25), hi=(3.0, 2.5, 5.0))


def scatter_scene(pt, ctx, g, in_lights_list):
    ramp = GR.Ramp(**SC_RAMP)
    spec = SceneSpec()
    smoke = spec.add("mat_medium_grid", SC_RAMP["scale"], SC_ALBEDO, g, ramp.grid.values, SC_RAMP["lo"], SC_RAMP["hi"])
    lm = spec.add("mat_light", spec.add("tex_solid_rgb", *SC_EMISSION))
    spec.add("world_add_light" if in_lights_list else "world_add_object", spec.add("quad", *SC_QUAD, lm))
    spec.add("set_camera_medium", smoke)
    spec.add("world_build")
    c = SC_CAM
    spec.camera = default_camera(width=c["width"], spp=1, vfov=c["vfov"], look_from=c["look_from"], look_at=c["look_at"], focal_length=1.0,
                                 defocus_angle=0.0, blur_strength=0.0, env_color=(0.0, 0.0, 0.0), max_depth=2)
    return build(pt, ctx, spec)[:2]


@pytest.mark.parametrize("g", [0.0, 0.6])
def test_single_scattering_matches_quadrature(pt, ctx, g):
    """max_depth = 2 through an unbounded ramp grid: no camera ray meets the quad, so the expectation is the single-scattering integral
    int sigma_s(x) T(o, x) int_quad ph T(x, y) G dA dd alone, with the closed-form optical depth of a ramp."""
    c = SC_CAM
    fr = R.camera_frame(c["width"], 1.0, c["vfov"], c["look_from"], c["look_at"], (0.0, 1.0, 0.0), 1.0)
    H, W = fr["height"], c["width"]
    o, d = pixel_rays(fr, W)
    ramp = GR.Ramp(**SC_RAMP)
    S = GR.single_scatter_quad(o, d, ramp, g, SC_QUAD, 32, 40, 20.0)
    S2 = GR.single_scatter_quad(o, d, ramp, g, SC_QUAD, 64, 80, 20.0)
    expected = (S2[:, None] * np.array(SC_ALBEDO) * np.array(SC_EMISSION)).reshape(H, W, 3)
    results = {}
    for name, in_list in (("lights list", True), ("plain object", False)):
        gs, cam = scatter_scene(pt, ctx, g, in_list)
        if name == "lights list":
            hits = gs.intersect(np.concatenate([o, d, np.zeros((len(d), 1))], axis=1))
            assert (hits[:, 0] == 0.0).all()                             # no direct term in this frame
        batches = np.stack([gs.render(cam, 3 + in_list, k * 256, (k + 1) * 256)[0] / 256 for k in range(16)])
        gs.close()
        results[name] = batches
        mean, sem = batches.mean(axis=0), batches.std(axis=0, ddof=1) / 4.0
        z = (mean - expected) / sem
        g_ = batches.mean(axis=(1, 2))
        zg = (g_.mean(axis=0) - expected.mean(axis=(0, 1))) / (g_.std(axis=0, ddof=1) / 4.0)
        quad_err = np.abs(S / S2 - 1.0).max()
        print(f"g {g}, {name}: quadrature changes by {quad_err:.3g} on doubling the nodes; smallest relative standard error {np.min(sem / expected):.3g}")
        assert quad_err * 100.0 < np.min(sem / expected)                 # the quadrature's error is two orders below the noise
        accept(z, zg)
    a, b = results["lights list"], results["plain object"]
    se2 = lambda x: x.var(axis=0, ddof=1) / len(x)
    z = (a.mean(axis=0) - b.mean(axis=0)) / np.sqrt(se2(a) + se2(b))
    ga, gb = a.mean(axis=(1, 2)), b.mean(axis=(1, 2))
    zg = (ga.mean(axis=0) - gb.mean(axis=0)) / np.sqrt(se2(ga) + se2(gb))
    assert np.isfinite(z).all() and (np.abs(z) > 4.0).mean() < 0.01 and np.abs(zg).max() < 4.0, (np.abs(z).max(), zg)


# ---- 8. a constant grid is the homogeneous medium, statistically ----------------------------------------------------------
def test_constant_grid_equals_homogeneous_medium(pt, ctx):
    scale, cval = 1.6, 0.75

    def scene(grid):
        spec = SceneSpec()
        if grid:
            med = spec.add("mat_medium_grid", scale, (0.9, 0.7, 0.5), 0.3, np.full((3, 4, 5), cval, dtype=np.float32), (-2.0, -1.0, -1.5), (2.5, 3.0, 2.0))   # contains the boundary
        else:
            med = spec.add("mat_medium", scale * cval, (0.9, 0.7, 0.5), 0.3)
        spec.add("world_add_object", spec.add("sphere", 0.9, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), med))
        floor = spec.add("mat_diffuse", spec.add("tex_solid_rgb", 0.8, 0.8, 0.8), -1)
        spec.add("world_add_object", spec.add("quad", (-60.0, -0.2, -60.0), (0.0, 0.0, 120.0), (120.0, 0.0, 0.0), floor))   # fills the frame
        lm = spec.add("mat_light", spec.add("tex_solid_rgb", 8.0, 7.0, 6.0))
        spec.add("world_add_light", spec.add("quad", (-1.0, 3.5, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), lm))
        spec.add("world_build")
        spec.camera = default_camera(width=24, spp=1, look_from=(0.0, 3.0, -4.0), look_at=(0.0, 0.6, 0.0), vfov=40.0, focal_length=1.0, defocus_angle=0.0,
                                     env_color=(0.3, 0.4, 0.5), max_depth=20)
        return build(pt, ctx, spec)[:2]

    res = {}
    for grid in (True, False):
        gs, cam = scene(grid)
        res[grid] = np.stack([gs.render(cam, 11 + grid, k * 256, (k + 1) * 256)[0] / 256 for k in range(16)])
        gs.close()
    a, b = res[True], res[False]
    se2 = lambda x: x.var(axis=0, ddof=1) / len(x)
    assert (se2(a) + se2(b) > 0.0).all()                                 # every pixel sees the floor or the ball: none is a constant
    z = (a.mean(axis=0) - b.mean(axis=0)) / np.sqrt(se2(a) + se2(b))
    ga, gb = a.mean(axis=(1, 2)), b.mean(axis=(1, 2))
    zg = (ga.mean(axis=0) - gb.mean(axis=0)) / np.sqrt(se2(ga) + se2(gb))
    print(f"constant grid vs homogeneous: max |z| {np.abs(z).max():.2f}, share |z| > 4 {(np.abs(z) > 4).mean():.4f}, image z {zg}")
    assert np.isfinite(z).all() and (np.abs(z) > 4.0).mean() < 0.01 and np.abs(zg).max() < 4.0, (np.abs(z).max(), zg)


# ---- 9. structure ------------------------------------------------------------------------------------------------------------
def smoke_cornell(pt, ctx, grids=True):
    """Scene 3 with an unbounded plume as the camera medium, a ball of grid smoke and a ball of homogeneous fog: lights, instances,
    every branch of the rule. grids = False: the same objects and handles with homogeneous media in the grid media's places."""
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 64, 6)
    if grids:
        plume = gs.mat_medium_grid(0.004, (0.9, 0.9, 0.9), 0.5, GR.smoke_plume(16), (-5.0, -5.0, -900.0), (560.0, 560.0, 560.0))
        smoke = gs.mat_medium_grid(0.02, (0.6, 0.7, 0.8), -0.3, random_values(31), (290.0, 310.0, 110.0), (470.0, 490.0, 290.0))
    else:
        plume = gs.mat_medium(0.004, (0.9, 0.9, 0.9), 0.5)
        smoke = gs.mat_medium(0.02, (0.6, 0.7, 0.8), -0.3)
    gs.world_add_object(gs.sphere(80.0, (380.0, 400.0, 200.0), (380.0, 400.0, 200.0), smoke))
    fog = gs.mat_medium(0.01, (0.8, 0.7, 0.6), 0.2)
    gs.world_add_object(gs.sphere(60.0, (150.0, 420.0, 250.0), (150.0, 420.0, 250.0), fog))
    gs.set_camera_medium(plume)
    gs.world_build()
    return gs, cam, plume


def test_structure_with_grid_media(pt, ctx):
    gs, cam, plume = smoke_cornell(pt, ctx)
    seed, n = 7, 6
    full, st = gs.render(cam, seed, 0, n, slots_per_pixel=1)
    plain = pt.Scene(ctx)
    pcam = plain.build_scene(3, 64, 6)
    base, st0 = plain.render(pcam, seed, 0, n, slots_per_pixel=1)
    aov0 = plain.render_aovs(pcam, seed, 0, 4)
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
    # AOVs do not change: the camera medium has no surface, and a grid medium's boundary is the first hit a homogeneous medium's is
    aov = gs.render_aovs(cam, seed, 0, 4)
    gs.set_camera_medium(-1)
    np.testing.assert_array_equal(gs.render_aovs(cam, seed, 0, 4), aov)
    gs.set_camera_medium(plume)
    hom, hcam, _ = smoke_cornell(pt, ctx, grids=False)
    np.testing.assert_array_equal(hom.render_aovs(hcam, seed, 0, 4), aov)
    hom.close()
    assert 0.0 < (aov[..., 6] != aov0[..., 6]).mean() < 0.3             # (the balls are in the frame)
    gs.set_sampler("sobol")                              # the Sobol forms: the same identities
    qfull, _ = gs.render(cam, seed, 0, n, slots_per_pixel=1)
    assert not np.array_equal(qfull, full)
    qparts = np.zeros_like(qfull)
    for s in range(n):
        gs.render(cam, seed, s, s + 1, accum=qparts, slots_per_pixel=1)
    np.testing.assert_array_equal(qparts, qfull)
    qdyn, _ = gs.render(cam, seed, 0, n)
    qfin = np.isfinite(qfull)
    np.testing.assert_allclose(qdyn[qfin], qfull[qfin], rtol=1e-12, atol=1e-12)
    gs.close()


def test_env_sampling_with_grid_media_is_refused(pt, ctx):
    gs = pt.Scene(ctx)
    gs.set_float_hdr(True)
    cam = gs.build_scene(6, 32, 2)
    gs.set_env_sampling(0.5)
    gs.render(cam, 1, 0, 1)                                  # fine without media
    smoke = gs.mat_medium_grid(0.1, (1.0, 1.0, 1.0), 0.0, random_values(41), (-5.0, -5.0, -5.0), (5.0, 5.0, 5.0))
    gs.world_build()
    gs.render(cam, 1, 0, 1)                                  # a medium nothing uses is not in effect
    gs.set_camera_medium(smoke)
    with pytest.raises(pt.PtError, match="participating media"):
        gs.render(cam, 1, 0, 1)
    gs.set_env_sampling(0.0)
    gs.render(cam, 1, 0, 1)
    cam.max_depth = 1 << 20                                  # the medium word's bounce field
    with pytest.raises(pt.PtError, match="max_depth"):
        gs.render(cam, 1, 0, 1)
    gs.close()


# ---- 10. the CLI -------------------------------------------------------------------------------------------------------------
def test_cli_smoke(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    common = ["-s", "3", "--width", "64", "--spp", "8", "--assets", pt.ASSET_DIR]

    def run(name, *extra):
        out = tmp_path / name
        r = subprocess.run([exe] + common + list(extra) + ["--out", str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return pt.decode_image_rgb8(str(out)).astype(np.float64)

    scale = 0.02
    mean_density = scale * float(GR.smoke_plume().astype(np.float64).mean())
    smoke = run("smoke.png", "--smoke", f"{scale},0.9,0.9,0.9,0.4")
    clear = run("clear.png")
    fog = run("fog.png", "--fog", f"{mean_density!r},0.9,0.9,0.9,0.4")
    d_clear, d_fog = np.abs(smoke - clear).mean(), np.abs(smoke - fog).mean()
    print(f"--smoke {scale} (mean density {mean_density:.3g}): mean |difference| {d_clear:.2f} against the clear render, {d_fog:.2f} against --fog")
    assert d_clear > 1.0 and d_fog > 1.0                                  # the plume is in the picture, and it is not a fog
    r = subprocess.run([exe, "-s", "6", "--width", "32", "--spp", "2", "--smoke", "0.1", "--sampler", "sobol", "--out", str(tmp_path / "s.png"), "--assets",
                        pt.ASSET_DIR], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe] + common + ["--smoke", "1000", "--out", str(tmp_path / "t.png")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 101 and "4096" in r.stderr                    # the design limit reaches the CLI as the library's refusal
