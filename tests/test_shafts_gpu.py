"""Light shafts on the GPU (pt_scene_set_punctual_media; the rule is in include/pt_amd.h): replays of whole renders from the
library's own probes (camera_probe, intersect, sampler_probe, medium_probe) plus the rule (tests/shafts_rule.py on top of medium_rule,
medium_grid_rule and punctual_rule), the physics against the single-scattering quadrature and a closed-form extinction, the new forms of
k_shade, "off means off", the refusals and limits, and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import medium_grid_rule as GR
import medium_rule as MR
import punctual_rule as PR
import shafts_rule as SH
import test_punctual_gpu as TP
import test_shafts_cpu as SC
from common import FORMS_H, FORMS_W, SceneSpec, _with_env, default_camera, forms_scene

pytestmark = pytest.mark.gpu

W = TP.W
FLOOR, OCCLUDER = TP.FLOOR, TP.OCCLUDER
ENV = (0.2, 0.25, 0.3)
# The fog cuboid of scene (a): above the floor, around the occluder. No edge of it lies on a diagonal of the frame, where the corner pixels'
# rays run, and it is low and narrow enough for the camera to see the floor beyond its +x side without looking through it: a shadow segment
# from there to the spot light crosses two boundaries and still has the depth for it (max_depth 5: segment 1, crossings 2 and 3).
BOX = ((-1.25, 0.3, -1.1), (0.6, 1.0, 1.1))
POINT_IN = ("light_point", (0.3, 0.7, -0.2), (12.0, 11.0, 10.0))            # inside the box
SPOT_OUT = ("light_spot", (-1.9, 1.0, 0.4), (1.5, 0.0, 0.1), 40.0, 60.0, (9.0, 8.0, 7.0))   # beside it, shining through it onto the floor beyond


def box_quads(lo, hi):
    """the six faces of a cuboid as (q, u, v), for the independent edge-margin test"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    e = np.diag(hi - lo)
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        out.append((lo, e[b], e[c]))
        out.append((lo + e[a], e[b], e[c]))
    return out


def make_scene(pt, ctx, quads, lights, medium=None, box=None, camera_medium=False, f=0.5, sampler="independent", max_depth=5, env=ENV, shafts=1, cam_kw=None):
    """Diffuse quads (primitive ids 0 ..), then the medium's cuboid (six more), no lights list. medium: ("homogeneous", density, albedo, g)
    or ("grid", scale, albedo, g, values). Returns (scene, camera, medium handle or -1)."""
    gs = pt.Scene(ctx)
    for q in quads:
        gs.world_add_object(gs.quad(q["q"], q["u"], q["v"], gs.mat_diffuse(gs.tex_solid_rgb(*q["albedo"]), -1)))
    mat = -1
    if medium is not None:
        mat = gs.mat_medium(*medium[1:]) if medium[0] == "homogeneous" else gs.mat_medium_grid(medium[1], medium[2], medium[3], medium[4], box[0], box[1])
        if box is not None and not camera_medium:
            gs.world_add_object(gs.cuboid(box[0], box[1], mat))
        if camera_medium:
            gs.set_camera_medium(mat)
    for call in lights:
        getattr(gs, call[0])(*call[1:])
    gs.set_punctual_fraction(f)
    gs.set_sampler(sampler)
    gs.set_punctual_media(shafts)
    gs.world_build()
    spec = SceneSpec()
    spec.camera = default_camera(**dict(TP.CAM if cam_kw is None else cam_kw, env_color=env, max_depth=max_depth))
    return gs, spec.make_camera(pt.Camera, []), mat


def replay(pt, ctx, gs, cam, quads, medium, mat, box, camera_medium, seed, spp, f, sampler, max_depth, env=ENV):
    """Every sample of the frame by the rule. The hits are the library's (intersect, one batch per depth), the draws its sampler's
    (sampler_probe), the free-flight distances its medium's (medium_probe); an independent ray / quad test gives every hit's distance to
    an edge. Returns dict: rad (P, S, 3), margin (P, S) — the smallest of: a hit's distance to an edge, |t - D'|, |d - t_end| —, and the
    counts the tests assert: crossings (the boundaries each resolved SHADOW segment crossed), blocked, visible, vertex_punctual."""
    sobol = sampler == "sobol"
    n = gs.punctual_count()
    recs = [PR.record(gs.punctual_light(k)) for k in range(n)]
    P, S, ND = W * W, spp, 128
    ps = np.stack(np.meshgrid(np.arange(P), np.arange(S), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
    cr = gs.camera_probe(cam, seed, ps)
    draws = np.concatenate([ctx.sampler_probe(sampler, seed, p, 0, S, 0, ND) for p in range(P)])          # (P * S, ND) from draw 0, pixel-major like ps
    units = PR.unit(draws)
    N = P * S
    grid = GR.Grid(medium[1], medium[4], box[0], box[1]) if medium is not None and medium[0] == "grid" else None
    albedo_m, g_m = (np.asarray(medium[2], dtype=np.float64), medium[3]) if medium is not None else (None, 0.0)
    bounded = medium is not None and not camera_medium
    all_quads = [(q["q"], q["u"], q["v"]) for q in quads] + (box_quads(*box) if bounded else [])
    if medium is not None and grid is None:                                # the free flight of every unit draw, by the device's own log
        flights = gs.medium_probe(mat, 1, units.reshape(-1)).reshape(units.shape)
    o, d, tm = cr[:, 0:3].copy(), cr[:, 3:6].copy(), cr[:, 6].copy()
    thr, rad = np.ones((N, 3)), np.zeros((N, 3))
    m = np.full(N, 0 if camera_medium else -1)                             # the path's medium: 0, or -1 = none
    bounce, draw = np.zeros(N, int), cr[:, 7].astype(int)
    shadow, k, crossed = np.zeros(N, bool), np.zeros(N, int), np.zeros(N, int)
    margin = np.full(N, np.inf)
    alive = np.ones(N, bool)
    out = dict(crossings=[], blocked=0, visible=0, hidden=0, vertex_punctual=0, surface_punctual=0, cut=0)
    envc = np.asarray(env, dtype=np.float64)
    p_light, p_punct, p_bsdf = PR.probabilities(f, False)

    def flight(i):                                                          # step 1 for path i in medium 0 over [0, t_end): (collided, distance)
        nonlocal draw
        if grid is not None:
            col, s, dr, _ = grid.track(o[i], d[i], t_end, lambda j: units[i, j], draw[i])
            draw[i] = dr
            return col, s
        dist = flights[i, draw[i]]
        draw[i] += 1
        return dist < t_end, dist

    def next_bounce(i):
        bounce[i] += 1
        if bounce[i] >= max_depth:
            alive[i] = False
            out["cut"] += int(shadow[i])

    for _ in range(max_depth):
        act = np.nonzero(alive)[0]
        if len(act) == 0:
            break
        hits = gs.intersect(np.concatenate([o[act], d[act], tm[act, None]], axis=1))
        t_ind, m_ind = PR.first_hit(o[act], d[act], all_quads)
        for row, i in enumerate(act):
            h = hits[row]
            is_hit = h[0] == 1.0
            t = h[1] if is_hit else np.inf
            assert is_hit == np.isfinite(t_ind[row]) and (not is_hit or abs(t - t_ind[row]) < 1e-9), (i, t, t_ind[row])
            if is_hit:
                margin[i] = min(margin[i], m_ind[row])
            prim, point, gn, sn = int(h[2]), h[6:9], h[9:12], h[12:15]
            boundary = is_hit and prim >= len(quads)
            assert draw[i] < ND - 40
            if m[i] == 0 and bounded and not is_hit:
                m[i] = -1                                                   # the lost crossing: no draw
            if shadow[i]:
                rec = recs[k[i]]
                dl = float(PR.shadow_distance(rec, o[i][None, :])[0])
                t_end = float(SH.segment_end(np.float64(t), np.float64(dl)))
                if np.isfinite(t) and np.isfinite(dl):
                    margin[i] = min(margin[i], abs(t - dl))
                if m[i] == 0:
                    col, dist = flight(i)
                    if grid is None:
                        margin[i] = min(margin[i], abs(dist - t_end))
                    if col:
                        out["blocked"] += 1
                        out["crossings"].append(crossed[i])
                        alive[i] = False
                        continue
                if boundary and t < dl:
                    m[i] = -1 if m[i] == 0 else 0
                    o[i] = point + (1e-3 * PR.signum(d[i] @ gn)) * gn
                    crossed[i] += 1
                    next_bounce(i)
                    continue
                if PR.visible(t, dl):
                    rad[i] = rad[i] + thr[i]
                    out["visible"] += 1
                else:
                    out["hidden"] += 1
                out["crossings"].append(crossed[i])
                alive[i] = False
                continue
            scatter = False
            if m[i] == 0:
                t_end = t
                col, dist = flight(i)
                if grid is None:
                    margin[i] = min(margin[i], abs(dist - t))
                scatter = col
            if scatter:
                x = o[i] + d[i] * dist
                r = units[i, draw[i]]                                       # the selector: read (bounce <= 5: no roulette)
                draw[i] += 1
                if r < p_light + p_punct:
                    k[i], used = PR.index_of_draws(draws[i, draw[i]:], n)
                    draw[i] += used
                    w, D, d2, E = PR.light_eval(recs[k[i]], x[None, :])
                    ph = MR.hg_phase(g_m, d[i] @ w[0])
                    thr2 = SH.vertex_throughput(thr[i], albedo_m, np.array([ph]), E, f, n)[0]
                    out["vertex_punctual"] += 1
                    if PR.branch_ends(d2, thr2[None, :])[0]:
                        alive[i] = False
                        continue
                    o[i], d[i], thr[i], shadow[i], crossed[i] = x, w[0] / np.linalg.norm(w[0]), thr2, True, 0
                else:
                    if sobol:
                        draw[i] = (draw[i] + 1) & ~1
                    u1, u2 = units[i, draw[i]], units[i, draw[i] + 1]
                    draw[i] += 2
                    if grid is None:                                        # the device's own direction and phase value
                        pr = gs.medium_probe(mat, 0, np.array([[u1, u2, *d[i]]]))[0]
                        w, ph = pr[0:3], pr[3]
                    else:
                        w = MR.hg_dir(g_m, u1, u2, d[i])
                        ph = MR.hg_phase(g_m, d[i] @ w)
                    pdf = p_bsdf * ph
                    assert pdf > 0.0 and np.isfinite(pdf)
                    thr[i] = thr[i] * (albedo_m * ph / pdf)
                    o[i], d[i] = x, w / np.linalg.norm(w)
                next_bounce(i)
                continue
            if not is_hit:
                rad[i] = rad[i] + thr[i] * envc
                alive[i] = False
                continue
            if boundary:
                m[i] = -1 if m[i] == 0 else 0
                o[i] = point + (1e-3 * PR.signum(d[i] @ gn)) * gn
                next_bounce(i)
                continue
            # a diffuse quad: no emission; the selector
            alb = np.asarray(quads[prim]["albedo"], dtype=np.float64)
            r = units[i, draw[i]]
            draw[i] += 1
            q = PR.LR.frame_to_z(sn)
            if r < p_light + p_punct:
                k[i], used = PR.index_of_draws(draws[i, draw[i]:], n)
                draw[i] += used
                w, D, d2, E = PR.light_eval(recs[k[i]], point[None, :])
                e = abs(PR.LR.quat_mul(q, w[0])[2]) * (alb / PR.PI)
                thr2 = PR.branch_throughput(thr[i], e, E[0], f, n)
                out["surface_punctual"] += 1
                if PR.branch_ends(d2, thr2[None, :])[0]:
                    alive[i] = False
                    continue
                o[i], d[i], thr[i], shadow[i], crossed[i] = PR.shadow_origin(point, gn, w[0]), w[0] / np.linalg.norm(w[0]), thr2, True, 0
            else:
                if sobol:
                    draw[i] = (draw[i] + 1) & ~1
                a, b = draws[i, draw[i]], draws[i, draw[i] + 1]
                draw[i] += 2
                phi = float(a >> np.uint64(12)) * (1.0 / 4503599627370496.0) * (2.0 * PR.PI)
                r2 = float(PR.unit(b))
                local = np.array([np.sqrt(r2) * np.cos(phi), np.sqrt(r2) * np.sin(phi), np.sqrt(1.0 - r2)])
                wd = PR.LR.quat_mul((-q[0], -q[1], -q[2], q[3]), local)
                lz = abs(local[2])
                assert lz > 1e-9                                            # (a direction in the surface's plane: the sampler would return None)
                thr[i] = thr[i] * ((lz * (alb / PR.PI)) / (p_bsdf * (lz / PR.PI) + 0.0))
                o[i], d[i] = PR.shadow_origin(point, gn, wd), wd / np.linalg.norm(wd)
            next_bounce(i)
    assert not alive.any()
    sh = lambda x: x.reshape(P, S, *x.shape[1:])
    out.update(rad=sh(rad), margin=sh(margin), crossings=np.asarray(out["crossings"]))
    return out


def sums(rp):
    acc = np.zeros_like(rp["rad"][:, 0])
    for s in range(rp["rad"].shape[1]):
        acc = acc + rp["rad"][:, s]
    return acc.reshape(W, W, 3)


def check_replay(pt, ctx, quads, lights, medium, box, camera_medium, sampler, seed=11, spp=4, f=0.5, max_depth=5):
    gs, cam, mat = make_scene(pt, ctx, quads, lights, medium, box, camera_medium, f, sampler, max_depth)
    acc, st = gs.render(cam, seed, 0, spp, slots_per_pixel=1)
    rp = replay(pt, ctx, gs, cam, quads, medium, mat, box, camera_medium, seed, spp, f, sampler, max_depth)
    print(f"{sampler}: margin {rp['margin'].min():.3e}; segments resolved {len(rp['crossings'])}: blocked {rp['blocked']} visible {rp['visible']} hidden {rp['hidden']} "
          f"cut by the depth bound {rp['cut']}; crossings {np.bincount(rp['crossings'], minlength=3)}; punctual at vertices {rp['vertex_punctual']}, at surfaces {rp['surface_punctual']}")
    TP.assert_no_sample_left_out(rp)
    assert st.samples == W * W * spp
    np.testing.assert_allclose(acc, sums(rp), rtol=1e-12, atol=0.0)        # (numpy's cos / sin / log stand in for the device's: not the last bit)
    dyn, dst = gs.render(cam, seed, 0, spp)
    assert (dst.samples, dst.segments) == (st.samples, st.segments)
    np.testing.assert_allclose(dyn, acc, rtol=1e-11, atol=1e-11)
    gs.close()
    return rp


# ---- 1. replays -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_replay_fog_box_point_inside_spot_outside(pt, ctx, sampler):
    """(a): shadow segments cross 0, 1 and 2 boundaries, and end blocked as well as visible"""
    rp = check_replay(pt, ctx, [FLOOR, OCCLUDER], [POINT_IN, SPOT_OUT], ("homogeneous", 0.9, (0.9, 0.8, 0.7), 0.3), BOX, False, sampler)
    counts = np.bincount(rp["crossings"], minlength=3)
    assert (counts[:3] >= 20).all(), counts
    assert rp["blocked"] >= 100 and rp["visible"] >= 100 and rp["vertex_punctual"] >= 100 and rp["surface_punctual"] >= 1000


@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_replay_unbounded_camera_medium(pt, ctx, sampler):
    """(b): an unbounded camera medium and a spot light"""
    rp = check_replay(pt, ctx, [FLOOR, OCCLUDER], [SPOT_OUT], ("homogeneous", 0.35, (0.9, 0.8, 0.7), -0.2), None, True, sampler)
    assert rp["blocked"] >= 100 and rp["visible"] >= 100 and rp["vertex_punctual"] >= 500 and (rp["crossings"] == 0).all()


@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_replay_grid_medium(pt, ctx, sampler):
    """(c): the fog box of (a) filled with a grid medium: the free flight of paths and SHADOW segments is medium_grid_rule's delta tracking"""
    values = np.random.default_rng(5).uniform(0.0, 1.0, size=(4, 4, 4)).astype(np.float32)
    rp = check_replay(pt, ctx, [FLOOR, OCCLUDER], [POINT_IN, SPOT_OUT], ("grid", 1.6, (0.9, 0.8, 0.7), 0.3, values), BOX, False, sampler)
    assert rp["blocked"] >= 50 and rp["visible"] >= 100 and rp["vertex_punctual"] >= 50 and (np.bincount(rp["crossings"], minlength=3)[:3] >= 10).all()


# ---- 2. physics -----------------------------------------------------------------------------------------------------------------------------
PW = 16
PCAM = dict(width=PW, aspect=1.0, vfov=40.0, look_from=tuple(SC.RAY_O), look_at=(0.0, 0.0, 1.0), vup=(0.0, 1.0, 0.0), blur_strength=0.0, defocus_angle=0.0,
            focal_length=1.0, env_color=(0.0, 0.0, 0.0))
WALL = dict(q=(-10.0, -10.0, SC.T_WALL), u=(20.0, 0.0, 0.0), v=(0.0, 20.0, 0.0), albedo=(0.0, 0.0, 0.0))
LIGHT_CALLS = {"point": ("light_point", tuple(SC.POINT["pos"]), (60.0, 50.0, 40.0)),
               "spot": ("light_spot", tuple(SC.SPOT["pos"]), tuple(SC.SPOT["pos"] + SC.SPOT_AXIS), 20.0, 40.0, (9.0, 8.0, 7.0))}


def batch_means(gs, cam, n_seeds=16, spp=256):
    return np.stack([gs.render(cam, seed, 0, spp)[0] / spp for seed in range(1, n_seeds + 1)])


def zscores(batches, want):
    mean, sem = batches.mean(axis=0), batches.std(axis=0, ddof=1) / np.sqrt(len(batches))
    with np.errstate(invalid="ignore", divide="ignore"):                   # (a pixel whose every sample is exactly 0: z is not used there)
        return (mean - want) / sem, mean, sem


@pytest.mark.parametrize("g", [0.0, 0.6])
@pytest.mark.parametrize("light", ["point", "spot"])
def test_single_scattering_equals_the_quadrature(pt, ctx, light, g):
    gs, cam, _ = make_scene(pt, ctx, [WALL], [LIGHT_CALLS[light]], ("homogeneous", SC.DENSITY, SC.ALBEDO, g), None, True, max_depth=2, env=(0.0, 0.0, 0.0), cam_kw=PCAM)
    rec = PR.record(gs.punctual_light(0))
    n = PW * PW
    rays = gs.camera_probe(cam, 1, np.stack([np.arange(n), np.zeros(n)], axis=1))
    np.testing.assert_array_equal(rays[:, :6], gs.camera_probe(cam, 2, np.stack([np.arange(n), np.full(n, 7.0)], axis=1))[:, :6])   # no jitter, no lens: one ray per pixel
    hit = gs.intersect(rays[:, :7])
    assert (hit[:, 0] == 1.0).all()
    near = np.array([SC.closest_approach(rays[i, 0:3], rays[i, 3:6], hit[i, 1], rec["pos"]) for i in range(n)])
    test = near >= 0.5
    assert test.sum() >= 100
    want = np.zeros((n, 3))
    for i in np.nonzero(test)[0]:
        want[i], change = SH.single_scatter_expected(rays[i, 0:3], rays[i, 3:6], hit[i, 1], SC.DENSITY, SC.ALBEDO, g, rec)
        assert change < 1e-8
    z, mean, sem = zscores(batch_means(gs, cam).reshape(16, n, 3), want)
    lit = test & (want[:, 0] > 1e-4 * want[test, 0].max())                   # (outside a spot's cone the expectation and every sample are exactly 0)
    print(f"{light} g={g}: {test.sum()} test pixels, {lit.sum()} lit; max |z| {np.abs(z[lit]).max():.2f}; image mean {mean[lit].mean(axis=0)} expected {want[lit].mean(axis=0)}")
    assert lit.sum() >= 50 and (np.abs(z[lit]) < 5.0).all()
    assert not mean[test & (want[:, 0] == 0.0)].any()
    total, total_sem = mean[lit].mean(axis=0), np.sqrt((sem[lit] ** 2).sum(axis=0)) / lit.sum()
    assert (total_sem < 0.03 * want[lit].mean(axis=0)).all() and (np.abs(total - want[lit].mean(axis=0)) < 5.0 * total_sem).all()   # a zero estimate cannot pass
    gs.close()


def test_pure_extinction_in_closed_form(pt, ctx):
    """A slab of fog of albedo (0, 0, 0) around a lit floor: the floor's radiance is the fog-free punctual value (a / pi) cos I / d^2 times
    exp(-sigma (l_camera + l_shadow)), the lengths of the camera ray and the shadow ray inside the slab. max_depth 4: the camera ray enters the
    slab (1), the floor bounce (2), the shadow segment leaves the slab (3)."""
    sigma, top, power, lpos = 0.6, 1.5, (40.0, 40.0, 40.0), np.array([0.3, 2.4, -0.2])
    slab = ((-8.0, -0.5, -8.0), (8.0, top, 8.0))
    gs, cam, _ = make_scene(pt, ctx, [FLOOR], [("light_point", tuple(lpos), power)], ("homogeneous", sigma, (0.0, 0.0, 0.0), 0.0), slab, False, max_depth=4, env=(0.0, 0.0, 0.0))
    cam.image_width = PW
    n = PW * PW
    rays = gs.camera_probe(cam, 1, np.stack([np.arange(n), np.zeros(n)], axis=1))
    free = pt.Scene(ctx)                                                    # the same floor without the slab: where the camera rays land
    free.world_add_object(free.quad(FLOOR["q"], FLOOR["u"], FLOOR["v"], free.mat_diffuse(free.tex_solid_rgb(*FLOOR["albedo"]), -1)))
    free.world_build()
    hit = free.intersect(rays[:, :7])
    free.close()
    on = hit[:, 0] == 1.0
    assert on.sum() >= 200
    x = hit[:, 6:9]
    L = lpos[None, :] - x
    d2 = PR.dot(L, L)
    w = L / np.sqrt(d2)[:, None]
    clear = (np.asarray(FLOOR["albedo"]) / np.pi)[None, :] * (w[:, 1] * (power[0] / (4.0 * np.pi)) / d2)[:, None]
    l_cam, l_sh = top / np.abs(rays[:, 4]), top / w[:, 1]
    want = np.where(on[:, None], clear * np.exp(-sigma * (l_cam + l_sh))[:, None], 0.0)
    z, mean, sem = zscores(batch_means(gs, cam).reshape(16, n, 3), want)
    print(f"{on.sum()} floor pixels; attenuation {np.exp(-sigma * (l_cam + l_sh))[on].min():.3f} .. {np.exp(-sigma * (l_cam + l_sh))[on].max():.3f}; max |z| {np.abs(z[on]).max():.2f}")
    assert (np.abs(z[on]) < 5.0).all() and not mean[~on].any()
    total, total_sem = mean[on].mean(axis=0), np.sqrt((sem[on] ** 2).sum(axis=0)) / on.sum()
    assert (total_sem < 0.03 * want[on].mean(axis=0)).all() and (np.abs(total - want[on].mean(axis=0)) < 5.0 * total_sem).all()
    gs.close()


def test_fraction_does_not_change_the_mean(pt, ctx):
    gs, cam, _ = make_scene(pt, ctx, [FLOOR, OCCLUDER], [POINT_IN, SPOT_OUT], ("homogeneous", 0.9, (0.9, 0.8, 0.7), 0.3), BOX, False, max_depth=8, env=(0.0, 0.0, 0.0))
    cam.image_width, cam.blur_strength = 64, 0.5
    spp, frames = 256, {}
    for f in (0.25, 0.75):
        gs.set_punctual_fraction(f)
        frames[f] = [gs.render(cam, seed, 0, spp)[0] / spp for seed in (1, 2)]
    N = 64 * 64
    var = {f: (a - b).reshape(N, 3).var(axis=0, ddof=1) for f, (a, b) in frames.items()}
    mean = {f: ((a + b) / 2.0).reshape(N, 3).mean(axis=0) for f, (a, b) in frames.items()}
    sigma = np.sqrt((var[0.25] + var[0.75]) / (4.0 * N))
    z = (mean[0.25] - mean[0.75]) / sigma
    print(f"frame means {mean[0.25]} (f = 0.25) {mean[0.75]} (f = 0.75), sigma {sigma}, z {z}")
    assert (mean[0.25] > 0.01).all() and (np.abs(z) < 5.0).all(), z
    gs.close()


# ---- 3. every new form launches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["independent", "sobol"])
@pytest.mark.parametrize("lights", [True, False], ids=["lights", "nolights"])
@pytest.mark.parametrize("mode", ["MED", "HET"])
def test_every_light_shaft_form(pt, ctx, mode, lights, sampler):
    spec = forms_scene(mode, lights)
    gs = pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    unlit, _ = gs.render(cam, 7, 0, 4, slots_per_pixel=1)
    gs.light_point((0.5, 3.0, 0.5), (200.0, 180.0, 160.0))
    gs.light_spot((-2.0, 3.5, -1.0), (0.0, 0.0, 0.0), 20.0, 40.0, (30.0, 30.0, 40.0))
    gs.light_directional((0.2, -1.0, 0.3), (1.0, 0.9, 0.8))
    gs.set_punctual_media(1)
    gs.world_build()
    gs.set_sampler(sampler)
    forced = lambda v, fn: _with_env({"PT_EXPERIMENT": "1", "PT_SHADE_VARIANT": str(v)}, fn)
    ref, rst = gs.render(cam, 7, 0, 4, slots_per_pixel=1)
    assert rst.samples == FORMS_W * FORMS_H * 4
    fin = np.isfinite(ref)
    assert fin.mean() >= 0.99 and (sampler == "sobol" or (ref != unlit)[fin].mean() > 0.3)       # the lights are in the picture
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
        np.testing.assert_allclose(dl[msk][fin[msk]], ref[msk][fin[msk]], rtol=1e-11, atol=1e-11)
    ada, counts, ast = gs.render_adaptive(cam, 7, 2, 6, 0.05)
    assert ast.samples == int(counts.sum()) and counts.min() >= 2 and counts.max() <= 6
    gs.close()


# ---- 4. off means off ------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(pt, ctx):
    fog = ("homogeneous", 0.9, (0.9, 0.8, 0.7), 0.3)
    # only media in effect
    gs, cam, _ = make_scene(pt, ctx, [FLOOR, OCCLUDER], [], fog, BOX, False, shafts=0)
    off, ost = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    gs.set_punctual_media(1)
    on, nst = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    np.testing.assert_array_equal(on, off)
    assert nst.segments == ost.segments
    # both in effect, the option off: today's refusal, from every entry point; on: it renders (no rebuild in between)
    gs.light_point(*POINT_IN[1:])
    gs.world_build()
    gs.set_punctual_media(0)
    px = np.arange(10, dtype=np.uint32)
    for fn in (lambda: gs.render(cam, 2, 0, 8, slots_per_pixel=1), lambda: gs.render(cam, 2, 0, 8), lambda: gs.render_pixels(cam, 2, px, 0, 2), lambda: gs.render_adaptive(cam, 2, 2, 4, 0.1)):
        with pytest.raises(pt.PtError, match="punctual lights together with participating media or a glass interior are not supported"):
            fn()
    gs.set_punctual_media(1)
    lit, lst = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    assert np.isfinite(lit).all() and (lit != off).mean() > 0.3 and lst.samples == W * W * 8
    gs.render(cam, 2, 0, 8); gs.render_pixels(cam, 2, px, 0, 2); gs.render_adaptive(cam, 2, 2, 4, 0.1)
    gs.close()
    # only punctual lights in effect
    gs, cam, _ = make_scene(pt, ctx, [FLOOR, OCCLUDER], [POINT_IN, SPOT_OUT], shafts=0)
    off, ost = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    gs.set_punctual_media(1)
    on, nst = gs.render(cam, 2, 0, 8, slots_per_pixel=1)
    np.testing.assert_array_equal(on, off)
    assert nst.segments == ost.segments and on.any()
    gs.close()


# ---- 5. refusals and limits with the option on ----------------------------------------------------------------------------------------------
def test_refusals_with_the_option_on(pt, ctx):
    fog = ("homogeneous", 0.9, (0.9, 0.8, 0.7), 0.3)

    def base(extra):
        gs = pt.Scene(ctx)
        gs.world_add_object(gs.quad(FLOOR["q"], FLOOR["u"], FLOOR["v"], gs.mat_diffuse(gs.tex_solid_rgb(*FLOOR["albedo"]), -1)))
        gs.world_add_object(gs.cuboid(BOX[0], BOX[1], gs.mat_medium(*fog[1:])))
        gs.light_point(*POINT_IN[1:])
        gs.set_punctual_media(1)
        spec = SceneSpec()
        spec.camera = default_camera(**dict(TP.CAM, env_color=ENV, max_depth=4))
        cam = spec.make_camera(pt.Camera, [])
        extra(gs, cam)
        gs.world_build()
        return gs, cam

    def interior(gs, cam):
        glass = gs.mat_glass(gs.tex_solid_rgb(1.0, 1.0, 1.0), gs.tex_solid_f(0.05), 0.0, 1.5)
        gs.mat_glass_set_interior(glass, gs.mat_medium(0.5, (0.8, 0.8, 0.8), 0.0))
        gs.world_add_object(gs.sphere(0.3, (1.5, 0.5, 1.5), (1.5, 0.5, 1.5), glass))

    def tinted(gs, cam):
        gs.set_camera_medium(gs.mat_medium_tinted(0.2, (0.9, 0.8, 0.7), 0.0, (0.3, 0.1, 0.6)))

    def env(gs, cam):
        cam.env_is_map, cam.env_tex = 1, gs.tex_image_rgbf32(np.random.default_rng(1).uniform(0.1, 1.0, size=(4, 8, 3)).astype(np.float32))
        gs.set_env_sampling(0.5)

    def lse(gs, cam):
        gs.world_add_light(gs.sphere(0.2, (1.0, 2.0, 0.0), (1.0, 2.0, 0.0), gs.mat_light(gs.tex_solid_rgb(5.0, 5.0, 5.0))))
        gs.set_light_sampling("exact")

    def dsp(gs, cam):
        glass = gs.mat_glass(gs.tex_solid_rgb(1.0, 1.0, 1.0), gs.tex_solid_f(0.05), 0.0, 1.5)
        gs.mat_glass_set_dispersion(glass, 30.0)
        gs.world_add_object(gs.sphere(0.3, (1.5, 0.5, 1.5), (1.5, 0.5, 1.5), glass))

    def motion(gs, cam):
        box = gs.cuboid((0.0, 0.0, 0.0), (0.3, 0.3, 0.3), gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1))
        gs.world_add_object(gs.instance_moving(box, (0.0, 1.0, 0.0), 0.0, 0.0, (1.5, 0.5, 1.5), (1.7, 0.5, 1.5)))

    for extra, word in ((interior, "interior"), (tinted, "tinted"), (env, "environment importance sampling"), (lse, "exact light sampling"), (dsp, "dispersion"), (motion, "otion")):
        gs, cam = base(extra)
        px = np.arange(10, dtype=np.uint32)
        for fn in (lambda: gs.render(cam, 1, 0, 2, slots_per_pixel=1), lambda: gs.render(cam, 1, 0, 2), lambda: gs.render_pixels(cam, 1, px, 0, 2)):
            with pytest.raises(pt.PtError) as e:
                fn()
            assert word in str(e.value), (word, str(e.value))
        gs.close()
    # the layout's bound on max_depth
    gs, cam = base(lambda gs, cam: None)
    cam.max_depth = 256
    with pytest.raises(pt.PtError, match="at most 255"):
        gs.render(cam, 1, 0, 1, slots_per_pixel=1)
    cam.max_depth = 255
    deep, _ = gs.render(cam, 1, 0, 1, slots_per_pixel=1)
    assert np.isfinite(deep).all() and deep.any()
    cam.max_depth = 256
    gs.set_punctual_media(0)                                               # without the option: today's refusal, not the bound
    with pytest.raises(pt.PtError, match="not supported"):
        gs.render(cam, 1, 0, 1, slots_per_pixel=1)
    gs.set_punctual_media(1)
    gs.clear_punctual_lights()
    gs.world_build()
    gs.render(cam, 1, 0, 1, slots_per_pixel=1)                             # without the lights the bound is gone
    gs.close()


def test_a_full_list_and_the_last_medium_handle_fit_the_word(pt, ctx):
    """2048 lights, and a medium whose handle is high: the index and medium fields of the bounce word at large values"""
    gs = pt.Scene(ctx)
    gs.world_add_object(gs.quad(FLOOR["q"], FLOOR["u"], FLOOR["v"], gs.mat_diffuse(gs.tex_solid_rgb(*FLOOR["albedo"]), -1)))
    for _ in range(3000):
        gs.mat_diffuse(0, -1)
    fog = gs.mat_medium(0.9, (0.9, 0.8, 0.7), 0.3)
    assert fog > 3000
    gs.world_add_object(gs.cuboid(BOX[0], BOX[1], fog))
    for i in range(2048):
        gs.light_point((0.3 + 1e-4 * i, 1.1, -0.2), (12.0, 11.0, 10.0))
    gs.set_punctual_media(1)
    gs.world_build()
    spec = SceneSpec()
    spec.camera = default_camera(**dict(TP.CAM, env_color=ENV, max_depth=5))
    cam = spec.make_camera(pt.Camera, [])
    acc, st = gs.render(cam, 4, 0, 4, slots_per_pixel=1)
    dyn, dst = gs.render(cam, 4, 0, 4)
    assert np.isfinite(acc).all() and acc.any() and (dst.samples, dst.segments) == (st.samples, st.segments)
    np.testing.assert_allclose(dyn, acc, rtol=1e-11, atol=1e-11)
    gs.close()


# ---- 6. the CLI -------------------------------------------------------------------------------------------------------------------------------
def test_cli_light_shafts(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    out = tmp_path / "shafts.png"
    args = [exe, "-s", "3", "--width", "32", "--spp", "16", "--fog", "0.002,0.9,0.9,0.9,0.3", "--spot-light", "278,540,278,278,0,278,15,25,3e6,3e6,3e6", "--out", str(out),
            "--assets", pt.ASSET_DIR]
    r = subprocess.run(args + ["--light-shafts"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = pt.decode_image_rgb8(str(out)).astype(np.float64)
    assert img.shape[1] == 32 and np.isfinite(img).all() and img.mean() > 2.0
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--light-shafts" in r.stderr
    r = subprocess.run([exe, "-s", "3", "--width", "32", "--spp", "4", "--smoke", "0.01", "--sun", "0.2,-1,0.3,3,3,3", "--light-shafts", "--sampler", "sobol",
                        "--out", str(tmp_path / "sun.png"), "--assets", pt.ASSET_DIR], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
