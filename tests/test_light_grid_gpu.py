"""The light grid on the GPU (pt_scene_set_punctual_selection kind 1; the rule is in include/pt_amd.h): the table the build
kernel writes and the selection K3 makes against the numpy rule (tests/light_grid_rule.py) through pt_punctual_probe, replays of whole
renders in the manner of tests/test_punctual_gpu.py, the variance of a row of lamps against the uniform selection's, the mean against the
uniform selection's, every PLT and light-shaft form, "off means off", and the refusals."""
import os
import subprocess

import numpy as np
import pytest

import light_grid_rule as LG
import punctual_rule as PR
import sampler_rule as SR
import test_punctual_gpu as TP
from common import FORMS_H, FORMS_W, GOLDEN_DIR, SceneSpec, _with_env, default_camera, forms_scene

pytestmark = pytest.mark.gpu

W = TP.W
FLOOR, OCCLUDER, CEILING = TP.FLOOR, TP.OCCLUDER, TP.CEILING
SPOT = ("light_spot", (-0.6, 1.5, 0.4), (-0.2, 0.0, 0.1), 20.0, 35.0, (9.0, 8.0, 7.0))
SUN = ("light_directional", (0.3, -1.0, 0.2), (3.0, 2.5, 2.0))
BOX = (-2.0, 0.0, -2.0, 2.0, 3.0, 2.0)


def seven_lights():
    rng = np.random.default_rng(7)
    return [TP.POINT, SPOT, SUN] + [("light_point", tuple(rng.uniform((-2.0, 0.2, -2.0), (2.0, 2.8, 2.0))), tuple(rng.uniform(1.0, 30.0, 3))) for _ in range(4)]


def many_points(n, seed=64):
    rng = np.random.default_rng(seed)
    return [("light_point", tuple(rng.uniform((-1.9, 1.2, -1.9), (1.9, 2.8, 1.9))), tuple(rng.uniform(5.0, 40.0, 3))) for _ in range(n)]


def grid_scene(pt, ctx, quads, lights, dims=(0, 0, 0), box=None, f=0.5, sampler="independent", max_depth=2):
    gs, cam, order = TP.make_scene(pt, ctx, quads, lights, f, sampler=sampler, max_depth=max_depth)
    gs.set_punctual_selection("grid")
    gs.set_punctual_grid(*dims, box=box)
    gs.world_build()
    return gs, cam, order


def records16(gs):
    return np.stack([gs.punctual_light(k) for k in range(gs.punctual_count())])


def rule_table(gs):
    dims, box = gs.punctual_grid()
    return dims, box, LG.table(records16(gs), box, dims)


# ---- 1. the probe equals the rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["4x3x5, 7 lights", "2x2x2, 2048 lights"])
def test_table_equals_the_rule_bit_for_bit(pt, ctx, case):
    if case.startswith("4x3x5"):
        gs, _, _ = grid_scene(pt, ctx, [FLOOR, OCCLUDER], seven_lights(), (4, 3, 5), BOX)
    else:
        gs, _, _ = grid_scene(pt, ctx, [FLOOR, OCCLUDER], [TP.POINT, SPOT, SUN] + many_points(2045), (2, 2, 2), BOX)
    dims, box, T = rule_table(gs)
    assert (dims, tuple(box)) == ((4, 3, 5) if case.startswith("4x3x5") else (2, 2, 2), BOX)
    cells, n = T.shape
    ck = np.stack(np.meshgrid(np.arange(cells), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 2)
    got = gs.punctual_probe(3, ck).reshape(cells, n)
    assert got.tobytes() == T.tobytes(), np.argwhere(got != T)[:5]
    assert got[0].tobytes() == pt.punctual_grid_row(records16(gs), box, dims, 0).tobytes()      # the host twin holds the same row
    assert (got[:, -1] == 1.0).all() and (np.diff(got, axis=1) >= 0.0).all()
    for bad in ([[cells, 0]], [[0, n]], [[-1, 0]], [[0.5, 0]]):
        with pytest.raises(pt.PtError, match="cell of the built grid"):
            gs.punctual_probe(3, bad)
    gs.close()


@pytest.mark.parametrize("n_lights", [7, 2048])
def test_selection_equals_the_rule(pt, ctx, n_lights):
    lights = seven_lights() if n_lights == 7 else [TP.POINT, SPOT, SUN] + many_points(2045)
    gs, _, _ = grid_scene(pt, ctx, [FLOOR, OCCLUDER], lights, (4, 3, 5) if n_lights == 7 else (2, 2, 2), BOX)
    dims, box, T = rule_table(gs)
    m = 1 << 16
    rng = np.random.default_rng(16)
    pts = rng.uniform((-2.6, -0.4, -2.6), (2.6, 3.4, 2.6), (m, 3))
    a, b, _, _ = LG.cell_geometry(box, dims)
    faces = np.concatenate([a, b])[rng.integers(0, 2 * len(a), 4096)]
    pts[:4096] = np.where(rng.random((4096, 3)) < 0.7, faces, pts[:4096])
    pts[4096:4100] = [[np.nan, 0.0, 0.0], [np.inf, 1.0, 1.0], [-np.inf, -np.inf, 0.0], [1e300, 1.0, -1e300]]
    pts[4100:4100 + min(n_lights, 64)] = records16(gs)[:64, 1:4]          # at the lights: d2 = 0
    got = gs.punctual_probe(2, pts)
    v = SR.independent_u64(0, np.arange(m), 0, 0)                          # the draw of (seed 0, pixel i, sample 0), draw 0 ...
    for i in (0, 1, 777, m - 1):                                           # ... as the library's own probe hands it out
        assert int(ctx.sampler_probe("independent", 0, i, 0, 1, 0, 1)[0, 0]) == int(v[i])
    cell, k, p = LG.select(box, dims, T, pts, PR.unit(v))
    assert (got[:, 0] == cell).all() and (got[:, 1] == k).all() and got[:, 2].tobytes() == p.tobytes()
    assert (got[:, 3] == 1.0).all()                                        # exactly one draw
    assert len(np.unique(cell)) == len(T) and len(np.unique(k)) >= min(n_lights, 500)
    recs = records16(gs)
    for kk in np.unique(k):
        sel = k == kk
        with np.errstate(over="ignore", invalid="ignore"):                 # (the far points: 1e300 squared)
            want = PR.eval7(PR.record(recs[kk]), pts[sel])
        assert ((got[sel, 4:11] == want) | (np.isnan(want) & np.isnan(got[sel, 4:11]))).all(), kk    # (a NaN's sign is not the rule's: inf - inf at the far points)
    gs.close()


def test_probe_needs_the_grid(pt, ctx):
    gs, _, _ = TP.make_scene(pt, ctx, [FLOOR], [TP.POINT])
    for which, arr in ((2, [[0.0, 0.0, 0.0]]), (3, [[0.0, 0.0]])):
        with pytest.raises(pt.PtError, match="light grid"):
            gs.punctual_probe(which, arr)
    with pytest.raises(pt.PtError, match="not in effect"):
        gs.punctual_grid()
    assert gs.punctual_probe(0, [[0.0, 0.0, 0.0]]).shape == (1, 9)
    gs.close()


# ---- 2. whole-render replay ------------------------------------------------------------------------------------------------------------------
def replay(pt, ctx, gs, cam, order, seed, samples, f, sampler="independent"):
    """tests/test_punctual_gpu.py's replay with the light grid's selection: the expected radiance of every (pixel, sample) of a scene of
    diffuse quads without a lights list under a black environment at max_depth = 2, from the library's own probes plus the two rules."""
    assert not any(q.get("emission") for q in order)
    recs16 = records16(gs)
    recs = [PR.record(r) for r in recs16]
    dims, box, T = rule_table(gs)
    P, S = W * W, len(samples)
    ps = np.stack(np.meshgrid(np.arange(P), np.asarray(samples), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
    cr = gs.camera_probe(cam, seed, ps)
    hit = gs.intersect(cr[:, :7])
    c0 = int(cr[0, 7])
    assert (cr[:, 7] == c0).all()
    draws = np.concatenate([ctx.sampler_probe(sampler, seed, p, int(samples[0]), S, c0, 2) for p in range(P)])     # the selector draw, then u
    N = P * S
    rad = np.zeros((N, 3))
    margin = np.full(N, np.inf)
    occluded, beyond = np.zeros(N, bool), np.zeros(N, bool)
    kk, pp = np.full(N, -1), np.zeros(N)
    missed = hit[:, 0] == 0.0
    prim = hit[:, 2].astype(int)
    albedo = np.array([order[p]["albedo"] if not missed[i] else (0.0, 0.0, 0.0) for i, p in enumerate(prim)])
    point, gn, sn = hit[:, 6:9], hit[:, 9:12], hit[:, 12:15]
    branch = np.where(missed, -1, PR.branch_of(PR.unit(draws[:, 0]), f, False))
    quads = [(q["q"], q["u"], q["v"]) for q in order]
    rows = np.nonzero(branch == 1)[0]
    _, kk[rows], pp[rows] = LG.select(box, dims, T, point[rows], PR.unit(draws[rows, 1]))
    for k in np.unique(kk[rows]):
        rec = recs[k]
        r = rows[kk[rows] == k]
        w, D, d2, E = PR.light_eval(rec, point[r])
        e = np.abs(PR.LR.quat_mul(PR.LR.frame_to_z(sn[r]), w)[..., 2])[:, None] * (albedo[r] / PR.PI)
        thr2 = LG.branch_throughput(np.ones(3), e, E, f, pp[r])
        ends = PR.branch_ends(d2, thr2)
        o = PR.shadow_origin(point[r], gn[r], w)
        t, m = PR.first_hit(o, w, quads)
        dl = PR.shadow_distance(rec, o)
        vis = PR.visible(t, dl)
        rad[r] = np.where((~ends & vis)[:, None], thr2, 0.0)
        both = np.isfinite(t) & np.isfinite(dl)
        gap = np.abs(np.where(both, t, 0.0) - np.where(both, dl, np.inf))
        margin[r] = np.where(ends, np.inf, np.minimum(m, gap))
        occluded[r] = ~ends & ~vis
        beyond[r] = ~ends & vis & np.isfinite(t)
    sh = lambda x: x.reshape(P, S, *x.shape[1:])
    return dict(rad=sh(rad), branch=sh(branch), k=sh(kk), p=sh(pp), margin=sh(margin), occluded=sh(occluded), beyond=sh(beyond))


@pytest.mark.parametrize("sampler", ["independent", "sobol"])
@pytest.mark.parametrize("lights", ["one of each kind", "64 points"])
def test_replay(pt, ctx, lights, sampler):
    spp, seed, f = 8, 11, 0.5
    calls = [TP.POINT, SPOT, SUN] if lights == "one of each kind" else many_points(64)
    gs, cam, order = grid_scene(pt, ctx, [FLOOR, OCCLUDER, CEILING], calls, f=f, sampler=sampler)
    dims, box = gs.punctual_grid()
    assert dims == LG.auto_dims(box, len(calls)) == (16, 12, 16)
    np.testing.assert_array_equal(box, [-2.0, 0.0, -2.0, 2.0, 3.0, 2.0])                     # the union of the three quads' boxes
    acc, st = gs.render(cam, seed, 0, spp, slots_per_pixel=1)
    rp = replay(pt, ctx, gs, cam, order, seed, range(spp), f, sampler)
    TP.assert_no_sample_left_out(rp)
    np.testing.assert_allclose(acc, TP.sums(rp), rtol=1e-12, atol=0.0)
    punct = rp["branch"] == 1
    assert set(np.unique(rp["k"][punct])) == set(range(len(calls))) and rp["occluded"].sum() >= 50 and rp["beyond"].sum() >= 50
    assert rp["p"][punct].min() >= 0.125 / len(calls) * (1.0 - 1e-12) and rp["p"][punct].max() > 2.0 / len(calls)
    assert st.samples == W * W * spp
    dyn, dst = gs.render(cam, seed, 0, spp)
    assert dst.slots_per_pixel == 0 and dst.samples == st.samples and dst.segments == st.segments
    np.testing.assert_allclose(dyn, acc, rtol=1e-11, atol=1e-11)
    gs.close()


# ---- 3. the full list ------------------------------------------------------------------------------------------------------------------------
def test_a_full_list_replays(pt, ctx):
    """2048 lights on the 2 x 2 x 2 grid: the longest row, the index field of the bounce word at its largest"""
    calls = [("light_point", (0.3 + 1e-4 * i, 1.7, -0.2 + 1e-3 * (i % 37)), (40.0, 40.0, 40.0)) for i in range(2048)]
    gs, cam, order = grid_scene(pt, ctx, [FLOOR, OCCLUDER], calls, (2, 2, 2))
    acc, st = gs.render(cam, 4, 0, 4, slots_per_pixel=1)
    rp = replay(pt, ctx, gs, cam, order, 4, range(4), 0.5)
    assert rp["k"].max() > 1900
    ok = (rp["margin"] >= 1e-6).all(axis=1).reshape(W, W)
    assert ok.mean() > 0.95
    np.testing.assert_allclose(acc[ok], TP.sums(rp)[ok], rtol=1e-12, atol=0.0)
    dyn, _ = gs.render(cam, 4, 0, 4)
    np.testing.assert_allclose(dyn, acc, rtol=1e-11, atol=1e-11)
    gs.close()


# ---- 4. a row of lamps: the variance ---------------------------------------------------------------------------------------------------------
LAMPS = [("light_point", (-8.0 + 16.0 * (k + 0.5) / 32, 0.4, 0.0), (4.0 * PR.PI, 4.0 * PR.PI, 4.0 * PR.PI)) for k in range(32)]      # I = 1
STRIP = dict(q=(-8.0, 0.0, -1.0), u=(16.0, 0.0, 0.0), v=(0.0, 0.0, 2.0), albedo=(1.0, 1.0, 1.0))
STRIP_BOX, STRIP_DIMS = (-8.0, 0.0, -1.0, 8.0, 0.4, 1.0), (16, 1, 2)


def strip_scene(pt, ctx, kind, n_lamps=32):
    lamps = LAMPS if n_lamps == 32 else [("light_point", (-8.0 + 16.0 * (k + 0.5) / n_lamps, 0.4, 1e-3 * (k % 7)), (1.0, 1.0, 1.0)) for k in range(n_lamps)]
    gs, _, order = TP.make_scene(pt, ctx, [STRIP], lamps)
    if kind == 1:
        gs.set_punctual_selection("grid")
        gs.set_punctual_grid(*(STRIP_DIMS if n_lamps == 32 else (2, 2, 2)), box=STRIP_BOX)
        gs.world_build()
    spec = SceneSpec()
    # from above, the strip fills the frame: 48 x 6 pixels over 16 x 2 (the frame's half height at distance 4 is 0.98 < 1)
    spec.camera = default_camera(**dict(TP.CAM, width=48, aspect=8.0, vfov=27.5, look_from=(0.0, 4.0, 0.0), max_depth=2))
    return gs, spec.make_camera(pt.Camera, [])


def test_row_of_lamps_variance(pt, ctx):
    """The scene of the CPU test's enumeration. A sample's conditional mean, given its first hit x, is sum_k e E_k (nothing occludes, the BSDF
    branch brings nothing at max_depth 2 under a black environment). The squared error of the pixel sums against the summed means, kind 1
    over kind 0: the rule predicts 0.17 (tests/test_light_grid_cpu.py); the bound 0.3 is the issue's, for an estimate from ~10^4 samples."""
    spp, err = 16, {}
    for kind in (0, 1):
        gs, cam = strip_scene(pt, ctx, kind)
        P = cam.image_width * 6
        ps = np.stack(np.meshgrid(np.arange(P), np.arange(spp), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
        recs = [PR.record(gs.punctual_light(k)) for k in range(32)]
        err[kind] = 0.0
        for seed in (3, 4):                                                 # two frames of 48 x 6 x 16 = 4608 samples each: about 10^4
            hit = gs.intersect(gs.camera_probe(cam, seed, ps)[:, :7])
            assert (hit[:, 0] == 1.0).all()
            x = hit[:, 6:9]
            mean = np.zeros(len(x))
            for rec in recs:
                w, D, d2, E = PR.light_eval(rec, x)
                mean += (w[:, 1] / PR.PI) * E[:, 0]
            acc, st = gs.render(cam, seed, 0, spp, slots_per_pixel=1)
            assert acc.shape == (6, 48, 3) and st.samples == P * spp
            err[kind] += float(((acc[..., 0].reshape(P) - mean.reshape(P, spp).sum(axis=1)) ** 2).sum())
            rel = abs(acc[..., 0].sum() - mean.sum()) / mean.sum()
            print(f"kind {kind} seed {seed}: squared error of the pixel sums so far {err[kind]:.5g}, frame sum off by {rel:.3%}")
        gs.close()
    print(f"ratio {err[1] / err[0]:.4f}")
    assert err[1] / err[0] < 0.3


def test_row_of_lamps_full_list(pt, ctx):
    gs, cam = strip_scene(pt, ctx, 1, 2048)
    assert gs.punctual_grid()[0] == (2, 2, 2)
    acc, st = gs.render(cam, 3, 0, 4)
    assert np.isfinite(acc).all() and (acc > 0.0).mean() > 0.9 and st.samples == 48 * 6 * 4
    gs.close()


# ---- 5. the mean is unchanged ----------------------------------------------------------------------------------------------------------------
def welch(batches):
    """Welch's z per channel between the frame means of two lists of frames"""
    m = {k: np.array([b.reshape(-1, 3).mean(axis=0) for b in v]) for k, v in batches.items()}
    z = (m[0].mean(axis=0) - m[1].mean(axis=0)) / np.sqrt(m[0].var(axis=0, ddof=1) / len(m[0]) + m[1].var(axis=0, ddof=1) / len(m[1]))
    print(f"frame means {m[0].mean(axis=0)} (uniform) {m[1].mean(axis=0)} (grid), z {z}")
    return z, m


def batches_of(gs, cam, n=16, spp=16):
    out = {}
    for kind in (0, 1):
        gs.set_punctual_selection(kind)
        gs.world_build()
        out[kind] = [gs.render(cam, 100 + s, 0, spp)[0] / spp for s in range(n)]
    return out


def test_mean_is_unchanged_in_a_closed_scene(pt, ctx):
    gs = pt.Scene(ctx)
    wall = lambda q, u, v, c: gs.world_add_object(gs.quad(q, u, v, gs.mat_diffuse(gs.tex_solid_rgb(*c), -1)))
    wall((-1.0, 0.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (0.7, 0.7, 0.7))       # floor
    wall((-1.0, 2.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (0.7, 0.7, 0.7))       # ceiling
    wall((-1.0, 0.0, -1.0), (0.0, 2.0, 0.0), (0.0, 0.0, 2.0), (0.7, 0.2, 0.2))       # left
    wall((1.0, 0.0, -1.0), (0.0, 2.0, 0.0), (0.0, 0.0, 2.0), (0.2, 0.7, 0.2))        # right
    wall((-1.0, 0.0, 1.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.7, 0.7, 0.7))        # back
    wall((-0.5, 0.8, -0.3), (0.9, 0.0, 0.0), (0.0, 0.0, 0.8), (0.5, 0.5, 0.5))       # an occluder: the cells under it lie in the shadow of the lamps above
    rng = np.random.default_rng(5)
    for i in range(8):                                                      # lamps above the occluder and two below it
        gs.light_point((rng.uniform(-0.8, 0.8), 1.7 if i < 6 else 0.4, rng.uniform(-0.8, 0.8)), tuple(rng.uniform(1.0, 6.0, 3)))
    for i in range(6):                                                      # narrow spots: most cells lie outside every cone
        pos = (rng.uniform(-0.8, 0.8), 1.9, rng.uniform(-0.8, 0.8))
        gs.light_spot(pos, (rng.uniform(-0.9, 0.9), 0.0, rng.uniform(-0.9, 0.9)), 8.0, 14.0, tuple(rng.uniform(2.0, 8.0, 3)))
    gs.light_spot((0.0, 1.0, -0.9), (0.0, 1.0, 0.9), 5.0, 30.0, (3.0, 3.0, 3.0))     # along the room
    gs.light_directional((0.2, -1.0, 0.1), (2.0, 2.0, 2.0))                          # a sun the ceiling blocks everywhere
    gs.set_punctual_grid(4, 4, 4)
    gs.world_build()
    assert gs.punctual_count() == 16 and {int(gs.punctual_light(k)[0]) for k in range(16)} == {0, 1, 2}
    spec = SceneSpec()
    spec.camera = default_camera(width=48, aspect=1.0, max_depth=4, vfov=50.0, look_from=(0.0, 1.0, -3.1), look_at=(0.0, 1.0, 0.0), vup=(0.0, 1.0, 0.0),
                                 blur_strength=0.5, defocus_angle=0.0, focal_length=1.0, env_color=(0.0, 0.0, 0.0))
    cam = spec.make_camera(pt.Camera, [])
    z, m = welch(batches_of(gs, cam))
    T = LG.table(records16(gs), gs.punctual_grid()[1], (4, 4, 4))
    p = LG.probabilities(T)
    floored = np.isclose(p, 0.125 / 16, rtol=1e-9).sum(axis=1)                        # per cell: the spots whose cone misses it keep the floor alone
    assert floored.mean() >= 3.0 and floored.max() >= 6 and floored.min() <= 1
    assert (m[0].mean(axis=0) > 0.01).all() and (np.abs(z) < 4.5).all(), z
    gs.close()


def test_mean_is_unchanged_in_a_fog_box(pt, ctx):
    import test_shafts_gpu as TS
    lights = [TS.SPOT_OUT, TS.POINT_IN, ("light_point", (-0.9, 0.5, 0.6), (6.0, 6.0, 6.0)), ("light_point", (1.2, 1.4, -0.8), (9.0, 8.0, 7.0))]
    gs, cam, _ = TS.make_scene(pt, ctx, [FLOOR, OCCLUDER], lights, medium=("homogeneous", 0.9, (0.9, 0.8, 0.7), 0.3), box=TS.BOX, env=(0.0, 0.0, 0.0))
    assert gs.punctual_media() == 1
    gs.set_punctual_grid(4, 2, 4)
    z, m = welch(batches_of(gs, cam))
    assert (m[0].mean(axis=0) > 0.01).all() and (np.abs(z) < 4.5).all(), z
    gs.close()


# ---- 6. every form ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["independent", "sobol"])
@pytest.mark.parametrize("lights", [True, False], ids=["lights", "nolights"])
@pytest.mark.parametrize("mode", ["PLAIN", "MED", "HET"])
def test_every_form_under_the_grid(pt, ctx, mode, lights, sampler):
    spec = forms_scene(mode, lights)
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    gs.light_point((0.5, 3.0, 0.5), (200.0, 180.0, 160.0))
    gs.light_spot((-2.0, 3.5, -1.0), (0.0, 0.0, 0.0), 20.0, 40.0, (30.0, 30.0, 40.0))
    gs.light_directional((0.2, -1.0, 0.3), (1.0, 0.9, 0.8))
    gs.light_point((-1.5, 1.0, 2.0), (60.0, 80.0, 100.0))
    gs.set_punctual_media(1 if mode != "PLAIN" else 0)
    gs.world_build()
    gs.set_sampler(sampler)
    uniform, _ = gs.render(cam, 7, 0, 4, slots_per_pixel=1)
    gs.set_punctual_selection("grid")
    gs.world_build()
    assert gs.punctual_grid()[0] == LG.auto_dims(gs.punctual_grid()[1], 4)
    forced = lambda v, fn: _with_env({"PT_EXPERIMENT": "1", "PT_SHADE_VARIANT": str(v)}, fn)
    ref, rst = forced(22, lambda: gs.render(cam, 7, 0, 4, slots_per_pixel=1))
    assert rst.shade_variant == 22 and rst.samples == FORMS_W * FORMS_H * 4
    fin = np.isfinite(ref)
    assert fin.mean() >= 0.99 and (ref != uniform)[fin].mean() > 0.05                          # the selection is in the picture
    sel = np.sort(np.random.default_rng(65).choice(FORMS_W * FORMS_H, size=65, replace=False)).astype(np.uint32)
    msk = np.zeros(FORMS_W * FORMS_H, bool)
    msk[sel] = True
    msk = msk.reshape(FORMS_H, FORMS_W)
    same = lambda a, b: ((a == b) | (np.isnan(a) & np.isnan(b))).all()
    for v in (22, 32):
        acc, st = forced(v, lambda: gs.render(cam, 7, 0, 4, slots_per_pixel=1))
        assert st.shade_variant == v and same(acc, ref) and (st.segments, st.samples) == (rst.segments, rst.samples), v
        out, st = forced(v, lambda: gs.render_pixels(cam, 7, sel, 0, 4, slots_per_pixel=1))
        assert st.shade_variant == v and st.samples == 65 * 4 and same(out[msk], ref[msk]) and not out[~msk].any(), v
        dyn, st = forced(v, lambda: gs.render(cam, 7, 0, 4))
        assert st.shade_variant == v and (st.segments, st.samples) == (rst.segments, rst.samples)
        np.testing.assert_allclose(dyn[fin], ref[fin], rtol=1e-11, atol=1e-11)
        dl, st = forced(v, lambda: gs.render_pixels(cam, 7, sel, 0, 4))
        assert st.samples == 65 * 4
        np.testing.assert_allclose(dl[msk][fin[msk]], ref[msk][fin[msk]], rtol=1e-11, atol=1e-11)
    gs.close()


# ---- 7. off means off ------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(pt, ctx):
    g = np.load(os.path.join(GOLDEN_DIR, "scene3_w64_spp16_seed1.npz"))
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 64, 16)
    assert gs.punctual_selection() == "uniform"
    gs.set_punctual_selection("grid")
    gs.world_build()                                                        # kind 1 without a punctual light: nothing new runs
    assert gs.punctual_selection() == "grid" and gs.punctual_count() == 0
    with pytest.raises(pt.PtError, match="not in effect"):
        gs.punctual_grid()
    acc, st = gs.render(cam, 1, 0, 16, slots_per_pixel=1)
    np.testing.assert_array_equal(acc, g["accum"])
    assert st.segments == int(g["segments"])
    gs.close()
    # set and set back, against a twin that never set it; the setting waits for the build
    twin, cam, _ = TP.make_scene(pt, ctx, [FLOOR, OCCLUDER, CEILING], seven_lights())
    want, wst = twin.render(cam, 2, 0, 8, slots_per_pixel=1)
    gs, _, _ = TP.make_scene(pt, ctx, [FLOOR, OCCLUDER, CEILING], seven_lights())
    gs.set_punctual_selection("grid")
    gs.set_punctual_grid(3, 3, 3)
    before, _ = gs.render(cam, 2, 0, 8, slots_per_pixel=1)                  # not built yet: still uniform
    np.testing.assert_array_equal(before, want)
    with pytest.raises(pt.PtError, match="not in effect"):
        gs.punctual_grid()
    gs.world_build()
    assert gs.punctual_grid()[0] == (3, 3, 3)
    grid, _ = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    assert (grid != want).mean() > 0.3
    gs.set_punctual_selection("uniform")
    gs.set_punctual_grid(5, 5, 5)
    still, _ = gs.render(cam, 2, 0, 8, slots_per_pixel=1)                   # the last build's grid stays until the next one
    np.testing.assert_array_equal(still, grid)
    assert gs.punctual_grid()[0] == (3, 3, 3) and gs.punctual_selection() == "uniform"
    gs.world_build()
    back, bst = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    np.testing.assert_array_equal(back, want)
    assert bst.segments == wst.segments
    with pytest.raises(pt.PtError, match="not in effect"):
        gs.punctual_grid()
    gs.close()
    twin.close()


def test_one_scene_walks_the_kinds(pt, ctx):
    """kind 0 -> 1 -> 0 across rebuilds with a changed light list, each state against a fresh twin"""
    lists = [seven_lights()[:3], seven_lights(), many_points(5)]
    gs, cam, _ = TP.make_scene(pt, ctx, [FLOOR, OCCLUDER, CEILING], [])
    for kind, calls in zip((0, 1, 0), lists):
        gs.clear_punctual_lights()
        for call in calls:
            getattr(gs, call[0])(*call[1:])
        gs.set_punctual_selection(kind)
        gs.world_build()
        twin, _, _ = (grid_scene if kind == 1 else TP.make_scene)(pt, ctx, [FLOOR, OCCLUDER, CEILING], calls)
        for kw in (dict(slots_per_pixel=1), {}):
            a, ast = gs.render(cam, 6, 0, 4, **kw)
            b, bst = twin.render(cam, 6, 0, 4, **kw)
            if kw:
                np.testing.assert_array_equal(a, b)
            else:
                np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-11)
            assert (ast.segments, ast.samples) == (bst.segments, bst.samples)
        if kind == 1:
            assert gs.punctual_grid()[0] == twin.punctual_grid()[0]
            ck = [[c, k] for c in (0, 100) for k in range(len(calls))]
            assert gs.punctual_probe(3, ck).tobytes() == twin.punctual_probe(3, ck).tobytes()
        twin.close()
    gs.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_setter_refusals(pt, ctx):
    gs = pt.Scene(ctx)
    for bad in (2, -1, "tree"):
        with pytest.raises(pt.PtError):
            gs.set_punctual_selection(bad)
        assert gs.punctual_selection() == "uniform"
    nan, inf = float("nan"), float("inf")
    gs.set_punctual_grid(2, 3, 4, box=(0, 0, 0, 1, 1, 1))
    for dims, box in (((0, 3, 4), None), ((2, 3, 65), None), ((2, 0, 0), None), ((2, 2, 2), (0, 0, 0, 1, nan, 1)), ((2, 2, 2), (0, 0, 0, inf, 1, 1)), ((2, 2, 2), (0, 2, 0, 1, 1, 1))):
        with pytest.raises(pt.PtError, match="set_punctual_grid|punctual_grid"):
            gs.set_punctual_grid(*dims, box=box)
    gs.world_add_object(gs.quad(FLOOR["q"], FLOOR["u"], FLOOR["v"], gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)))
    gs.light_point((0.0, 1.0, 0.0), (1.0, 1.0, 1.0))
    gs.set_punctual_selection("grid")
    gs.world_build()
    dims, box = gs.punctual_grid()                                          # the refused calls changed nothing
    assert dims == (2, 3, 4) and tuple(box) == (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    gs.set_punctual_grid(1, 1, 1, box=(0.5, 0.5, 0.5, 0.5, 0.5, 0.5))       # hi = lo is a box
    gs.world_build()
    assert gs.punctual_grid()[0] == (1, 1, 1)
    gs.close()


def test_build_refusals(pt, ctx):
    gs = pt.Scene(ctx)
    gs.world_add_object(gs.quad((1e308, 0.0, 0.0), (1e308, 0.0, 0.0), (0.0, 0.0, 1.0), gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)))   # its far edge is at +inf
    gs.world_add_object(gs.quad(FLOOR["q"], FLOOR["u"], FLOOR["v"], gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)))
    gs.light_point((0.0, 1.0, 0.0), (1.0, 1.0, 1.0))
    gs.set_punctual_selection("grid")
    with pytest.raises(pt.PtError, match="give one"):
        gs.world_build()
    with pytest.raises(pt.PtError, match="give one"):
        gs.set_punctual_grid(4, 4, 4)                                       # dims alone do not help
        gs.world_build()
    gs.close()
    gs, cam, _ = TP.make_scene(pt, ctx, [FLOOR], [TP.POINT])                # a given box need not be the world's
    gs.set_punctual_selection("grid")
    gs.set_punctual_grid(0, 0, 0, box=(-1.0, 0.0, -1.0, 1.0, 0.5, 0.0))
    gs.world_build()
    assert gs.punctual_grid()[0] == (16, 4, 8) and np.isfinite(gs.render(cam, 1, 0, 2)[0]).all()
    gs.close()
    gs, cam, _ = TP.make_scene(pt, ctx, [FLOOR], many_points(256))
    gs.set_punctual_selection("grid")
    gs.set_punctual_grid(64, 64, 64)                                        # 2^18 cells x 2^8 lights
    with pytest.raises(pt.PtError, match="2\\^25"):
        gs.world_build()
    with pytest.raises(pt.PtError):
        gs.render(cam, 1, 0, 1)                                             # (a failed build leaves the world unbuilt)
    gs.set_punctual_grid(64, 64, 32)                                        # exactly 2^25: the largest table
    gs.world_build()
    assert gs.punctual_grid()[0] == (64, 64, 32)
    ck = [[64 * 64 * 32 - 1, 255], [12345, 0]]
    dims, box = gs.punctual_grid()
    rows = np.stack([pt.punctual_grid_row(records16(gs), box, dims, int(c)) for c, _ in ck])
    assert (gs.punctual_probe(3, ck) == [rows[0, 255], rows[1, 0]]).all()
    gs.set_punctual_grid(0, 0, 0)                                           # automatic dims halve R until the table fits
    gs.world_build()
    assert gs.punctual_grid()[0] == LG.auto_dims(gs.punctual_grid()[1], 256)
    gs.close()


def test_cli_selection(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    base = [exe, "-s", "3", "--width", "32", "--spp", "2", "--point-light", "278,500,278,3e7,3e7,3e7", "--point-light", "100,300,100,1e6,1e6,1e6", "--assets", pt.ASSET_DIR]
    imgs = {}
    for sel in ("uniform", "grid", "grid,4,3,2"):
        out = tmp_path / (sel.replace(",", "_") + ".png")
        r = subprocess.run(base + ["--punctual-selection", sel, "--out", str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        imgs[sel] = pt.decode_image_rgb8(str(out))
    assert (imgs["grid"] != imgs["uniform"]).any() and (imgs["grid,4,3,2"] != imgs["uniform"]).any()
    r = subprocess.run(base + ["--punctual-selection", "grid,4,4", "--out", str(tmp_path / "bad.png")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stderr.strip()
