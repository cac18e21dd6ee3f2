"""First-hit AOVs (pt_render_aovs) and the a-trous denoiser (pt_denoise) on the GPU.

The AOVs are checked exactly: depth and hit counts against the oracle's per-sample traces (so AOV sample s traces render sample
s's camera ray), albedo and normal material by material on a scene of camera-facing quads. The denoiser is checked against a
numpy restatement of the rule in include/pt_amd.h on random inputs, for its exact properties, and for calibrated quality."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H5 = np.array([1.0 / 16.0, 0.25, 0.375, 0.25, 1.0 / 16.0])
K3 = np.array([0.25, 0.5, 0.25])


# ---- the rule, restated ------------------------------------------------------------------------------------------------
def lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def shifted(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx] where that is inside the image, else `fill`; and the in-image mask."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ok = np.zeros((h, w), dtype=bool)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        ok[y0:y1, x0:x1] = True
    return out, ok


def denoise_np(sum_a, n_a, sum_b, n_b, aov, n_aov, K=5, sigma_l=4.0, sigma_z=0.1):
    n_a, n_b, n_aov = float(n_a), float(n_b), float(n_aov)
    mu = (sum_a + sum_b) / (n_a + n_b)
    hits = aov[..., 7]
    fg = hits != 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(fg, aov[..., 6] / hits, 0.0)
        ln = np.sqrt(aov[..., 3] * aov[..., 3] + aov[..., 4] * aov[..., 4] + aov[..., 5] * aov[..., 5])
        N = np.where((ln > 0.0)[..., None], aov[..., 3:6] / ln[..., None], 0.0)
    a = np.maximum(aov[..., 0:3] / n_aov, 1e-3)
    c = mu / a
    d = lum((sum_a / n_a) / a) - lum((sum_b / n_b) / a)
    v = d * d * (n_a * n_b / ((n_a + n_b) * (n_a + n_b)))
    for k in range(K):
        s = 1 << k
        gs = np.zeros_like(v)
        gw = np.zeros_like(v)
        for j in range(-1, 2):
            for i in range(-1, 2):
                vq, ok = shifted(v, j, i, 0.0)
                fq, _ = shifted(fg, j, i, False)
                m = ok & fq
                kk = K3[j + 1] * K3[i + 1]
                gw = gw + np.where(m, kk, 0.0)
                gs = gs + np.where(m, kk * vq, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = gs / gw
        lp = lum(c)
        dl = sigma_l * np.sqrt(g) + 1e-10
        dz = sigma_z * z + 1e-10
        sw = np.zeros_like(v)
        sv = np.zeros_like(v)
        sc = np.zeros_like(c)
        for j in range(-2, 3):
            for i in range(-2, 3):
                cq, ok = shifted(c, s * j, s * i, 0.0)
                vq, _ = shifted(v, s * j, s * i, 0.0)
                zq, _ = shifted(z, s * j, s * i, 0.0)
                Nq, _ = shifted(N, s * j, s * i, 0.0)
                fq, _ = shifted(fg, s * j, s * i, False)
                m = ok & fq & fg
                with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                    e = np.exp(-(np.abs(lp - lum(cq)) / dl) - np.abs(z - zq) / dz)
                pw = np.maximum(0.0, N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1] + N[..., 2] * Nq[..., 2])
                for _ in range(7):
                    pw = pw * pw
                w = np.where(m, H5[i + 2] * H5[j + 2] * e * pw, 0.0)
                sw = sw + w
                sc = sc + w[..., None] * cq
                sv = sv + w * w * vq
        upd = fg & (sw > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(upd[..., None], sc / sw[..., None], c)
            v = np.where(upd, sv / (sw * sw), v)
    return np.where(fg[..., None], c * a, mu)


def random_inputs(w, h, seed, n_a=3, n_b=5, n_aov=4):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    hits = rng.integers(0, n_aov + 1, size=(h, w)).astype(np.float64)
    hits[rng.random((h, w)) < 0.5] = n_aov                                       # mostly full hits, some partial, some background
    base = np.stack([0.3 * np.sin(xx / 5.0), 0.3 * np.cos(yy / 7.0), np.ones_like(xx)], axis=-1)
    nrm = base / np.linalg.norm(base, axis=-1, keepdims=True) + 0.05 * rng.standard_normal((h, w, 3))
    depth = 3.0 + 0.05 * xx + 0.02 * yy + 0.1 * rng.random((h, w))
    alb = rng.uniform(0.05, 1.0, size=(h, w, 3))
    alb[rng.random((h, w, 3)) < 0.1] = 0.0                                         # zero-albedo channels
    aov = np.zeros((h, w, 8))
    aov[..., 0:3] = alb * n_aov
    aov[..., 3:6] = nrm * hits[..., None]
    aov[..., 6] = depth * hits
    aov[..., 7] = hits
    mean = 0.5 + 0.3 * np.sin((xx + yy)[..., None] / 9.0 + np.array([0.0, 1.0, 2.0]))
    sum_a = (mean + 0.2 * rng.standard_normal((h, w, 3))).clip(0.0, None) * n_a
    sum_b = (mean + 0.2 * rng.standard_normal((h, w, 3))).clip(0.0, None) * n_b
    return sum_a, n_a, sum_b, n_b, aov, n_aov


class DeviceBuffer:
    hip = None

    def __init__(self, host):
        if DeviceBuffer.hip is None:
            hip = C.CDLL("libamdhip64.so")
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipFree.argtypes = [C.c_void_p]
            DeviceBuffer.hip = hip
        self.nbytes, self.shape, self.dtype = host.nbytes, host.shape, host.dtype
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), host.nbytes) == 0
        assert self.hip.hipMemcpy(self.ptr, host.ctypes.data, host.nbytes, 1) == 0

    def get(self):
        out = np.empty(self.shape, self.dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0
        return out

    def free(self):
        self.hip.hipFree(self.ptr)


# ---- 1. AOV depth and hits against the oracle, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("scene_id,width", [(3, 24), (6, 32), (1, 24)])   # scene 1: defocus and moving spheres
def test_aov_depth_and_hits_match_oracle(pt, det, ctx, scene_images, scene_id, width):
    seed = 11
    gs = pt.Scene(ctx)
    for name, img in scene_images(scene_id).items():
        gs.register_image(name, img)
    cam = gs.build_scene(scene_id, width, 2)
    aov = gs.render_aovs(cam, seed, 0, 2)
    os_ = det.Scene()
    ocam = os_.build_scene(scene_id, width, 2, images=scene_images(scene_id))
    h = aov.shape[0]
    hits = np.zeros((h, width))
    depth = np.zeros((h, width))
    for p in range(h * width):
        for s in range(2):
            _, rec, _ = os_.trace_sample(ocam, seed, p, s)
            if len(rec) and rec[0][0] != 0.0:                                    # (rows past the recorded hits are zero; a hit has t >= 1e-3)
                hits[p // width, p % width] += 1.0
                depth[p // width, p % width] += rec[0][0]
    assert hits.sum() > 0
    np.testing.assert_array_equal(aov[..., 7], hits)
    np.testing.assert_array_equal(aov[..., 6], depth)
    miss = hits == 0
    np.testing.assert_array_equal(aov[miss][:, 0:3], 2.0)                          # a miss: albedo (1, 1, 1) per sample
    np.testing.assert_array_equal(aov[miss][:, 3:6], 0.0)
    os_.close()
    gs.close()


# ---- 2. albedo and normal by material -----------------------------------------------------------------------------------
def quad_scene(pt, ctx):
    """Ten camera-facing quads (5 x 2), one per material kind, plus a checker-textured diffuse and two mixes."""
    gs = pt.Scene(ctx)
    red, green, blue = (0.8, 0.1, 0.1), (0.1, 0.7, 0.2), (0.15, 0.25, 0.9)
    t_red, t_green, t_blue = gs.tex_solid_rgb(*red), gs.tex_solid_rgb(*green), gs.tex_solid_rgb(*blue)
    t_gold = gs.tex_solid_rgb(0.9, 0.6, 0.2)
    t_white = gs.tex_solid_rgb(0.9, 0.9, 0.9)
    rough = gs.tex_solid_f(0.3)
    checker = gs.tex_checker(0.5, t_red, t_white)
    one = (1.0, 1.0, 1.0)
    m_diffuse = gs.mat_diffuse(t_red)
    m_metal = gs.mat_metal(t_blue, rough)
    m_glass = gs.mat_glass(t_green, rough, 0.0, 1.5)
    m_princ = gs.mat_principled(t_gold, [0.2, 0.4, 0.0, 0.5, 0.0, 1.5, 0.0, 0.0, 0.5, 0.0, 1.0])
    m_light = gs.mat_light(gs.tex_solid_rgb(4.0, 4.0, 4.0))
    sheen = (0.2, 0.7, 0.3)
    m_sheen = gs.mat_sheen(sheen, 0.5)
    m_coat = gs.mat_clearcoat(0.5)
    m_mix = gs.mat_mix(0.3, m_diffuse, m_metal)
    m_inner = gs.mat_mix(0.6, gs.mat_diffuse(t_green), m_glass)
    m_nested = gs.mat_mix(0.25, m_sheen, m_inner)
    m_check = gs.mat_diffuse(checker)
    a = np.array
    expect = [a(red), a(blue), a(one), a((0.9, 0.6, 0.2)), a(one),
              a(sheen), a(one), (1.0 - 0.3) * a(red) + 0.3 * a(blue),
              (1.0 - 0.25) * a(sheen) + 0.25 * ((1.0 - 0.6) * a(green) + 0.6 * a(one)), None]
    mats = [m_diffuse, m_metal, m_glass, m_princ, m_light, m_sheen, m_coat, m_mix, m_nested, m_check]
    quads = []
    for k, m in enumerate(mats):
        cx, cy = -4.0 + 2.0 * (k % 5), 1.0 - 2.0 * (k // 5)
        q = gs.quad((cx - 0.8, cy - 0.8, 0.0), (1.6, 0.0, 0.0), (0.0, 1.6, 0.0), m)
        gs.world_add_object(q)
        if m == m_light:
            gs.world_add_light(q)
        quads.append(q)
    gs.world_build()
    cam = pt.Camera()
    cam.aspect_ratio, cam.image_width, cam.samples_per_pixel, cam.max_depth = 2.0, 160, 1, 8
    cam.vfov = 30.0
    cam.look_from[:], cam.look_at[:], cam.vup[:] = (0.0, 0.0, 10.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    cam.blur_strength, cam.focal_length, cam.defocus_angle = 1.0, 10.0, 0.0
    cam.env_color[:] = (0.1, 0.2, 0.3)
    cam.env_tex = -1
    return gs, cam, expect, red, (0.9, 0.9, 0.9)


def checker_first(p, inv_scale=2.0):
    s = sum(int(math.floor(c * inv_scale)) for c in p)
    return s % 2 == 0


def test_aov_albedo_and_normal_by_material(pt, ctx):
    gs, cam, expect, c_first, c_second = quad_scene(pt, ctx)
    aov = gs.render_aovs(cam, 3, 0, 1)
    d, h = pt.camera_init(cam)
    w = cam.image_width
    # rays through each pixel's centre and through points one pixel away (the camera's jitter reaches at most one pixel)
    offs = [(0.0, 0.0), (-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0), (1.0, 1.0)]
    rays = []
    for oy, ox in offs:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        tgt = d["pixel00"] + d["pixel_dv"] * (yy + oy)[..., None] + d["pixel_du"] * (xx + ox)[..., None]
        o = np.array(cam.look_from[:])
        r = np.zeros((h, w, 7))
        r[..., 0:3] = o
        r[..., 3:6] = tgt - o
        rays.append(r.reshape(-1, 7))
    hit = [gs.intersect(r).reshape(h, w, 15) for r in rays]
    checked = np.zeros(len(expect), dtype=int)
    for y in range(h):
        for x in range(w):
            c = hit[0][y, x]
            if c[0] == 0.0:
                continue
            if any(hh[y, x, 0] == 0.0 or hh[y, x, 2] != c[2] for hh in hit[1:]):
                continue                                                     # near a quad's edge
            k = int(round((c[6] + 4.0) / 2.0)) + (0 if c[7] > 0.0 else 5)        # the quad the hit point lies on
            if expect[k] is None:                                                # the checker: both cells must agree over the footprint
                parity = {checker_first(hh[y, x, 6:9]) for hh in hit}
                if len(parity) != 1:
                    continue
                want = np.array(c_first if parity.pop() else c_second)
            else:
                want = expect[k]
            np.testing.assert_array_equal(aov[y, x, 0:3], want, err_msg=f"material {k} at ({y}, {x})")
            np.testing.assert_array_equal(aov[y, x, 3:6], c[12:15], err_msg=f"normal of material {k} at ({y}, {x})")
            assert aov[y, x, 7] == 1.0 and aov[y, x, 6] > 0.0
            checked[k] += 1
    assert (checked >= 50).all(), checked
    miss = aov[..., 7] == 0
    assert miss.sum() > 100 and miss[0, 0] and miss[-1, -1]                        # the image's corners see only the environment
    np.testing.assert_array_equal(aov[miss][:, 0:3], 1.0)
    np.testing.assert_array_equal(aov[miss][:, 3:8], 0.0)
    gs.close()


# ---- 3. ranges add up, device and host agree, arguments are checked -------------------------------------------------------
def test_aov_ranges_add_and_device_agrees(pt, ctx):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 48, 4)
    full = gs.render_aovs(cam, 9, 0, 4)
    part = gs.render_aovs(cam, 9, 0, 2)
    gs.render_aovs(cam, 9, 2, 4, aov=part)
    np.testing.assert_allclose(part, full, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(full[..., 7], np.round(full[..., 7]))
    assert full[..., 7].max() == 4.0 and full[..., 7].min() >= 0.0
    # overwrite stores; the empty range adds nothing / stores zeros
    junk = np.full_like(full, 7.5)
    np.testing.assert_array_equal(gs.render_aovs(cam, 9, 0, 4, aov=junk, overwrite=True), full)
    keep = full.copy()
    np.testing.assert_array_equal(gs.render_aovs(cam, 9, 3, 3, aov=keep), full)
    np.testing.assert_array_equal(gs.render_aovs(cam, 9, 3, 3, aov=keep, overwrite=True), 0.0)
    # device accumulator: the same sums
    dev = DeviceBuffer(np.full_like(full, 1.25))
    gs.render_aovs(cam, 9, 0, 4, device_ptr=dev.ptr.value)
    np.testing.assert_array_equal(dev.get(), full + 1.25)
    gs.render_aovs(cam, 9, 0, 4, device_ptr=dev.ptr.value, overwrite=True)
    np.testing.assert_array_equal(dev.get(), full)
    dev.free()
    # bad arguments
    opts = pt.RenderOpts()
    assert pt.lib.pt_render_aovs(gs.handle, C.byref(cam), 9, 0, 4, None, C.byref(opts)) == -1
    with pytest.raises(pt.PtError, match="spp_end < spp_begin"):
        gs.render_aovs(cam, 9, 4, 2)
    unbuilt = pt.Scene(ctx)
    with pytest.raises(pt.PtError, match="not built"):
        unbuilt.render_aovs(cam, 9, 0, 1)
    unbuilt.close()
    gs.close()


# ---- 4. the denoiser matches the numpy restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(45, 29), (7, 300)])
@pytest.mark.parametrize("K,sigma_l,sigma_z", [(0, 4.0, 0.1), (1, 4.0, 0.1), (2, 1.5, 0.3), (3, 4.0, 0.1), (4, 0.7, 0.02), (5, 4.0, 0.1),
                                               (6, 2.0, 0.5)])
def test_denoise_matches_numpy_rule(pt, ctx, w, h, K, sigma_l, sigma_z):
    sa, na, sb, nb, aov, naov = random_inputs(w, h, seed=w * 1000 + h + K)
    assert (aov[..., 7] == 0).any() and ((aov[..., 7] > 0) & (aov[..., 7] < naov)).any() and (aov[..., 0:3] == 0).any()
    got = ctx.denoise(sa, na, sb, nb, aov, naov, iterations=K, sigma_l=sigma_l, sigma_z=sigma_z)
    want = denoise_np(sa, na, sb, nb, aov, naov, K, sigma_l, sigma_z)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)


# ---- 5. exact properties and argument checks ----------------------------------------------------------------------------
def test_denoise_background_and_noise_free(pt, ctx):
    sa, na, sb, nb, aov, naov = random_inputs(40, 33, seed=5)
    out = ctx.denoise(sa, na, sb, nb, aov, naov)
    bg = aov[..., 7] == 0
    mu = (sa + sb) / float(na + nb)
    np.testing.assert_array_equal(out[bg].view(np.uint64), mu[bg].view(np.uint64))
    # noise-free: both halves have the same mean (powers of two: the divisions are exact)
    m = np.abs(sa / na) + 0.01
    sa2, sb2 = m * 2.0, m * 4.0
    out2 = ctx.denoise(sa2, 2, sb2, 4, aov, naov, iterations=5)
    np.testing.assert_allclose(out2, (sa2 + sb2) / 6.0, rtol=1e-14, atol=0.0)


def test_denoise_bad_arguments(pt, ctx):
    sa, na, sb, nb, aov, naov = random_inputs(8, 8, seed=1)
    out = np.empty_like(sa)
    lib, hd = pt.lib, ctx.handle

    def call(w=8, h=8, a=sa, n_a=na, b=sb, n_b=nb, v=aov, n_v=naov, K=5, sl=4.0, sz=0.1, o=out, opts=True):
        ptr = lambda x: None if x is None else x.ctypes.data
        op = C.byref(pt.DenoiseOpts(K, sl, sz)) if opts else None
        return lib.pt_denoise(hd, w, h, ptr(a), n_a, ptr(b), n_b, ptr(v), n_v, op, ptr(o))

    assert call() == 0 and call(opts=False) == 0
    np.testing.assert_allclose(out, ctx.denoise(sa, na, sb, nb, aov, naov), rtol=0, atol=0)   # NULL opts = the defaults
    assert lib.pt_denoise(None, 8, 8, sa.ctypes.data, na, sb.ctypes.data, nb, aov.ctypes.data, naov, None, out.ctypes.data) == -1
    for bad in [dict(a=None), dict(b=None), dict(v=None), dict(o=None), dict(w=0), dict(h=0), dict(n_a=0), dict(n_b=0), dict(n_v=0),
                dict(K=11), dict(sl=0.0), dict(sl=-1.0), dict(sl=float("nan")), dict(sz=0.0), dict(sz=-0.5), dict(sz=float("nan"))]:
        assert call(**bad) == -1, bad
    assert call(K=10) == 0
    with pytest.raises(pt.PtError, match="pt_denoise"):
        ctx.denoise(sa, na, sb, nb, aov, naov, iterations=11)


# ---- 6. calibrated quality ----------------------------------------------------------------------------------------------
# Measured on one MI355X: denoised / raw relMSE 0.038 / 0.060 / 0.040 for these seeds; the red wall's mean green
# moves by 0.00126-0.00129 against the 8192-spp render. Bounds: the largest of each with 50 % margin.
QUALITY_RATIO_MAX = 0.09
BLEED_MAX = 0.002


def rel_mse(x, ref):
    return float(((x - ref) ** 2 / (ref ** 2 + 1e-2)).mean())


def test_denoise_quality_scene3(pt, ctx):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 128, 64)
    ref, _ = gs.render(cam, 1000, 0, 8192)
    ref /= 8192.0
    ratios, bleeds = [], []
    for seed in (1, 2, 3):
        a, _ = gs.render(cam, seed, 0, 32)
        b, _ = gs.render(cam, seed, 32, 64)
        aov = gs.render_aovs(cam, seed, 0, 16)
        dn = ctx.denoise(a, 32, b, 32, aov, 16)
        raw = (a + b) / 64.0
        ratios.append(rel_mse(dn, ref) / rel_mse(raw, ref))
        alb = aov[..., 0:3] / 16.0
        wall = (alb[..., 0] > 0.5) & (alb[..., 1] < 0.1) & (alb[..., 2] < 0.1)   # the red wall (0.65, 0.05, 0.05)
        assert wall.sum() > 500
        bleeds.append(abs(dn[wall][:, 1].mean() - ref[wall][:, 1].mean()))
    print(f"denoised/raw relMSE {ratios}, red wall green shift {bleeds}")
    assert max(ratios) <= QUALITY_RATIO_MAX, ratios
    assert max(bleeds) <= BLEED_MAX, bleeds
    gs.close()


# ---- 7. CLI -------------------------------------------------------------------------------------------------------------
def test_cli_denoise_matches_python_pipeline(pt, ctx, tmp_path):
    exe = os.path.join(ROOT, "thu-acg-f2024-path-tracer_amd", "pt_render")
    png = str(tmp_path / "dn.png")
    r = subprocess.run([exe, "-s", "3", "--width", "64", "--spp", "32", "--denoise", "--out", png, "--assets", pt.ASSET_DIR],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = pt.decode_image_rgb8(png)
    assert img.shape == (64, 64, 3)
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 64, 32)
    a, _ = gs.render(cam, 1, 0, 16)
    b, _ = gs.render(cam, 1, 16, 32)
    aov = gs.render_aovs(cam, 1, 0, 16)
    want = ctx.resolve_u8(ctx.denoise(a, 16, b, 16, aov, 16), 1)
    diff = np.abs(img.astype(int) - want.astype(int))
    assert (diff <= 1).mean() >= 0.999, (diff > 1).mean()
    gs.close()
