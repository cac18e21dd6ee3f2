"""The film stage on the GPU (pt_film_develop): exposure, glare, tone curves, HDR output.

Checked against the numpy restatement of the rule (tests/film_rule.py), for the properties that hold exactly, on host and on device
buffers, for every refusal, and through the CLI. The convolution kernel takes tiles of CONV_TX = 256 columns (csrc/pt_film.hip) with a
halo of the level's radius on either side; the long shapes below span more than two tiles plus both halos of the largest radius (384)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import film_rule as fr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV_TX = 256
R_LARGEST = 384                                    # sigma_0 = 8, L = 5: ceil(3 * 128)
LONG = 2 * CONV_TX + 2 * R_LARGEST + 21            # 1301: not a multiple of the tile or of the four columns a lane owns
SHAPES = [(45, 29), (7, 300), (300, 7), (1, 1), (LONG, 9), (9, LONG)]                 # (W, H)
BLOOMS = [(0.5, 1), (2.0, 3), (1.5, 6), (8.0, 5)]                                     # (sigma_0, L)
TONEMAPS = ["reference", "srgb", "reinhard", "aces"]


def frame(w, h, seed, n=4):
    """Sums of n samples whose means spread over [0, 6): dark pixels, pixels around every threshold used here, highlights."""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(0.0, 1.5, (h, w, 3)) * np.where(rng.random((h, w, 1)) < 0.15, 4.0, 1.0)
    return mean * n, n


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def check_rgb8(rgb8, v):
    """rgb8 equals the rule's quantiser on v except where v * 256 lies within 1e-6 of an integer above 0 (the device pow and numpy's
    may round to different sides there); returns how many channels were left out."""
    q = np.clip(v, 0.0, 0.999) * 256.0
    with np.errstate(invalid="ignore"):
        near = (q > 0.0) & (np.abs(q - np.round(q)) < 1e-6)
    np.testing.assert_array_equal(rgb8[~near], fr.quantise(v)[~near])
    return int(near.sum())


# ---- 1. the defaults are pt_resolve_u8 / pt_resolve_u8_counts ------------------------------------------------------------------
def test_defaults_equal_resolve_u8_byte_for_byte(pt, ctx):
    rng = np.random.default_rng(7)
    w, h, n = 61, 23, 12
    sums = rng.uniform(0.0, 2.5, (h, w, 3)) * n
    sums[rng.random((h, w, 3)) < 0.05] *= 40.0
    sums[3, 5] = (np.nan, -1.0, np.inf)
    sums[9, 60] = (1e300, 0.0, -np.inf)
    sums[22, 0] = (np.inf, np.nan, 1e300)
    hdr, rgb8 = ctx.film(sums, n)
    np.testing.assert_array_equal(rgb8, ctx.resolve_u8(sums, n))
    np.testing.assert_array_equal(bits(hdr), bits(np.fmax(sums * (1.0 / n), 0.0)))
    counts = rng.integers(1, 10, (h, w)).astype(np.uint32)
    hdr_c, rgb8_c = ctx.film(sums, counts=counts)
    np.testing.assert_array_equal(rgb8_c, ctx.resolve_u8_counts(sums, counts))
    np.testing.assert_array_equal(bits(hdr_c), bits(np.fmax(sums * (1.0 / counts.astype(np.float64))[..., None], 0.0)))
    assert len(np.unique(rgb8)) > 100 and rgb8.max() == 255 and rgb8.min() == 0
    # NULL options are the defaults too
    out = np.empty((h, w, 3), dtype=np.uint8)
    assert pt.lib.pt_film_develop(ctx.handle, w, h, sums.ctypes.data, n, None, None, None, out.ctypes.data) == 0
    np.testing.assert_array_equal(out, rgb8)


# ---- 2. against the numpy rule -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,levels", BLOOMS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_film_matches_numpy_rule(pt, ctx, w, h, sigma, levels):
    sums, n = frame(w, h, seed=w * 1000 + h)
    left_out = total = 0
    for thr in (0.0, 0.8):
        cache = {}

        def shared_glare(b, s0, nl):      # G depends on (T, sigma_0, L) alone: computed once for the strengths and curves below
            if "g" not in cache:
                cache["g"] = fr.glare(b, s0, nl)
            return cache["g"]

        for s, tonemap in itertools.product((0.3, 1.0), TONEMAPS):
            opts = dict(bloom_strength=s, bloom_threshold=thr, bloom_sigma=sigma, bloom_levels=levels, tonemap=tonemap, white=2.0, exposure_ev=0.5)
            hdr, rgb8 = ctx.film(sums, n, **opts)
            want_hdr, want_v = fr.film_np(sums, n, glare_of=shared_glare, **opts)
            np.testing.assert_allclose(hdr, want_hdr, rtol=1e-11, atol=1e-300, err_msg=str(opts))
            left_out += check_rgb8(rgb8, want_v)
            total += rgb8.size
    assert left_out <= 1e-3 * total, (left_out, total)


# ---- 3. exact properties --------------------------------------------------------------------------------------------------------
def test_no_glare_is_the_exposed_mean_bit_for_bit(pt, ctx):
    sums, n = frame(53, 31, seed=3)
    sums[4, 4] = (np.nan, -2.0, np.inf)
    for ev in (0.0, -1.0, 3.0):                     # integers: 2^ev is exact whatever exp2 the host has
        want = np.fmax((sums * (1.0 / n)) * np.exp2(ev), 0.0)
        hdr, _ = ctx.film(sums, n, exposure_ev=ev, tonemap="aces")
        np.testing.assert_array_equal(bits(hdr), bits(want))
    finite = sums.copy()
    finite[4, 4] = 1.0
    want = np.fmax(finite * (1.0 / n), 0.0)
    top = fr.lum(want).max()
    hdr, _ = ctx.film(finite, n, bloom_strength=0.7, bloom_threshold=top, bloom_sigma=1.0, bloom_levels=2)   # nothing is brighter than T
    np.testing.assert_array_equal(bits(hdr), bits(want))


def test_exposure_is_a_scale_of_the_sums(pt, ctx):
    sums, n = frame(70, 40, seed=4)
    glare = dict(bloom_strength=0.4, bloom_sigma=1.5, bloom_levels=3)
    a_hdr, a_rgb = ctx.film(sums, n, exposure_ev=1.0, bloom_threshold=1.0, tonemap="reinhard", **glare)
    b_hdr, b_rgb = ctx.film(2.0 * sums, n, exposure_ev=0.0, bloom_threshold=1.0, tonemap="reinhard", **glare)
    np.testing.assert_array_equal(bits(a_hdr), bits(b_hdr))
    np.testing.assert_array_equal(a_rgb, b_rgb)
    # ... and one stop less on the sums with T doubled is the same picture at twice the scale: every step is linear or a power of two
    c_hdr, _ = ctx.film(2.0 * sums, n, exposure_ev=0.0, bloom_threshold=2.0, **glare)
    d_hdr, _ = ctx.film(sums, n, exposure_ev=0.0, bloom_threshold=1.0, **glare)
    np.testing.assert_array_equal(bits(c_hdr), bits(2.0 * d_hdr))
    e_hdr, _ = ctx.film(sums, n, exposure_ev=1.0, bloom_threshold=2.0, **glare)
    np.testing.assert_array_equal(bits(e_hdr), bits(c_hdr))


def test_repeatable_and_flips_commute(pt, ctx):
    sums, n = frame(LONG // 2, 37, seed=5)
    opts = dict(bloom_strength=0.5, bloom_threshold=0.6, bloom_sigma=2.0, bloom_levels=4, tonemap="srgb")
    hdr, rgb8 = ctx.film(sums, n, **opts)
    hdr2, rgb82 = ctx.film(sums, n, **opts)
    np.testing.assert_array_equal(bits(hdr), bits(hdr2))
    np.testing.assert_array_equal(rgb8, rgb82)
    lr, _ = ctx.film(sums[:, ::-1], n, **opts)
    np.testing.assert_allclose(lr[:, ::-1], hdr, rtol=1e-13, atol=0.0)
    tb, _ = ctx.film(sums[::-1], n, **opts)
    np.testing.assert_allclose(tb[::-1], hdr, rtol=1e-13, atol=0.0)


# ---- 4. per-pixel counts --------------------------------------------------------------------------------------------------------
def test_counts_match_the_rule(pt, ctx):
    rng = np.random.default_rng(6)
    w, h = 83, 19
    counts = rng.integers(1, 10, (h, w)).astype(np.uint32)
    sums = rng.uniform(0.0, 2.0, (h, w, 3)) * counts[..., None]
    opts = dict(bloom_strength=0.6, bloom_threshold=0.5, bloom_sigma=1.0, bloom_levels=3, tonemap="aces", exposure_ev=-1.0)
    hdr, rgb8 = ctx.film(sums, counts=counts, **opts)
    want_hdr, want_v = fr.film_np(sums, counts, **opts)
    np.testing.assert_allclose(hdr, want_hdr, rtol=1e-11, atol=1e-300)
    assert check_rgb8(rgb8, want_v) <= 1e-3 * rgb8.size
    assert not np.allclose(hdr, fr.film_np(sums, 5, **opts)[0])             # the counts do matter


# ---- 5. device buffers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_counts", [False, True])
def test_on_device_equals_host_path(pt, ctx, with_counts):
    rng = np.random.default_rng(8)
    w, h, n = 300, 41, 6
    counts = rng.integers(1, 10, (h, w)).astype(np.uint32) if with_counts else None
    sums, _ = frame(w, h, seed=9, n=n)
    opts = dict(bloom_strength=0.25, bloom_sigma=2.0, bloom_levels=5, tonemap="aces")
    hdr, rgb8 = ctx.film(sums, n, counts=counts, **opts)
    d_sums, d_hdr, d_rgb = DeviceBuffer(sums), DeviceBuffer(np.zeros_like(hdr)), DeviceBuffer(np.zeros_like(rgb8))
    d_cnt = DeviceBuffer(counts) if with_counts else None
    ptrs = (w, h, d_sums.ptr.value, d_cnt.ptr.value if d_cnt else None, d_hdr.ptr.value, d_rgb.ptr.value)
    assert ctx.film(None, n, device_ptrs=ptrs, **opts) is None
    np.testing.assert_array_equal(bits(d_hdr.get()), bits(hdr))
    np.testing.assert_array_equal(d_rgb.get(), rgb8)
    np.testing.assert_array_equal(bits(d_sums.get()), bits(sums))           # the sums are read, never written
    # one output alone
    d_only = DeviceBuffer(np.zeros_like(rgb8))
    ctx.film(None, n, device_ptrs=(w, h, d_sums.ptr.value, d_cnt.ptr.value if d_cnt else None, None, d_only.ptr.value), **opts)
    np.testing.assert_array_equal(d_only.get(), rgb8)
    for b in (d_sums, d_hdr, d_rgb, d_only) + ((d_cnt,) if d_cnt else ()):
        b.free()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_return_minus_one_and_write_nothing(pt, ctx):
    w, h, n = 8, 6, 4
    sums, _ = frame(w, h, seed=10)
    counts = np.full((h, w), 3, dtype=np.uint32)
    zero_count = counts.copy()
    zero_count[2, 2] = 0
    hdr = np.full((h, w, 3), -7.0)
    rgb = np.full((h, w, 3), 77, dtype=np.uint8)
    lib, nan, inf = pt.lib, float("nan"), float("inf")

    def call(handle=ctx.handle, w=w, h=h, s=sums, n=n, c=None, o_hdr=hdr, o_rgb=rgb, null_opts=False, **opts):
        ptr = lambda x: None if x is None else x.ctypes.data
        op = None if null_opts else C.byref(pt.FilmOpts(**opts))
        return lib.pt_film_develop(handle, w, h, ptr(s), n, ptr(c), op, ptr(o_hdr), ptr(o_rgb))

    bad = [dict(handle=None), dict(s=None), dict(o_hdr=None, o_rgb=None), dict(w=0), dict(h=0), dict(n=0), dict(n=0, null_opts=True),
           dict(c=zero_count), dict(c=zero_count, n=0),
           dict(exposure_ev=nan), dict(exposure_ev=inf), dict(exposure_ev=100.5), dict(exposure_ev=-101.0),
           dict(tonemap=4), dict(white=nan), dict(white=inf), dict(white=5e-4), dict(white=-1.0),
           dict(bloom_strength=nan), dict(bloom_strength=-0.1), dict(bloom_strength=1.5),
           dict(bloom_threshold=nan), dict(bloom_threshold=-1.0), dict(bloom_threshold=inf),
           dict(bloom_sigma=nan), dict(bloom_sigma=0.25), dict(bloom_sigma=65.0),
           dict(bloom_levels=0), dict(bloom_levels=7), dict(bloom_sigma=8.0, bloom_levels=6), dict(bloom_sigma=64.0, bloom_levels=3),
           dict(bloom_strength=0.5, bloom_sigma=0.25),
           dict(bloom_strength=0.5, w=524281, h=1), dict(bloom_strength=0.5, w=1, h=524281)]   # beyond the convolution's launch grid: refused up front
    for b in bad:
        assert call(**b) == -1, b
        assert "pt_film_develop" in lib.pt_last_error().decode(), b
        assert (hdr == -7.0).all() and (rgb == 77).all(), b
    # the edges of every range are accepted
    for good in [dict(), dict(null_opts=True), dict(o_hdr=None), dict(o_rgb=None), dict(c=counts, n=0), dict(exposure_ev=100.0), dict(exposure_ev=-100.0),
                 dict(tonemap=3), dict(white=1e-3, tonemap=2), dict(bloom_strength=1.0, bloom_threshold=0.0, bloom_sigma=0.5, bloom_levels=1),
                 dict(bloom_strength=0.1, bloom_sigma=64.0, bloom_levels=2), dict(bloom_strength=0.1, bloom_sigma=4.0, bloom_levels=6)]:
        assert call(**good) == 0, (good, lib.pt_last_error())
    with pytest.raises(pt.PtError, match="pt_film_develop"):
        ctx.film(sums, n, tonemap=9)
    with pytest.raises(pt.PtError, match="pt_film_develop"):
        ctx.film(sums, counts=zero_count)


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_film_matches_python_pipeline(pt, ctx, tmp_path):
    exe = os.path.join(ROOT, "thu-acg-f2024-path-tracer_amd", "pt_render")
    png, hdr_file, plain = str(tmp_path / "f.png"), str(tmp_path / "f.hdr"), str(tmp_path / "p.png")
    base = [exe, "-s", "6", "--float-hdr", "--width", "96", "--spp", "16", "--assets", pt.ASSET_DIR]
    r = subprocess.run(base + ["--tonemap", "aces", "--bloom", "0.2", "--exposure", "-1", "--out", png, "--out-hdr", hdr_file],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    gs = pt.Scene(ctx)
    gs.set_float_hdr(True)
    cam = gs.build_scene(6, 96, 16)
    acc, _ = gs.render(cam, 1, 0, 16)
    assert (acc / 16.0).max() > 4.0                                          # radiances far above 1: what the stage is for
    hdr, rgb8 = ctx.film(acc, 16, tonemap="aces", bloom_strength=0.2, exposure_ev=-1.0)
    img = pt.decode_image_rgb8(png)
    assert img.shape == rgb8.shape
    diff = np.abs(img.astype(int) - rgb8.astype(int))
    assert (diff <= 1).mean() >= 0.999, (diff > 1).mean()
    back = pt.load_hdr_rgbf32(hdr_file).astype(np.float64)
    assert back.shape == hdr.shape
    max_c = hdr.max(axis=-1, keepdims=True)
    assert (np.abs(back - hdr) <= max_c / 128.0).all(), float((np.abs(back - hdr) / max_c).max())
    # without the film flags: the reference's PNG, byte for byte
    r = subprocess.run(base + ["--out", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(pt.decode_image_rgb8(plain), ctx.resolve_u8(acc, 16))
    assert not np.array_equal(pt.decode_image_rgb8(plain), img)
    gs.close()
