"""Pixel-list renders (pt_render_pixels) and adaptive sampling (pt_render_adaptive, pt_resolve_u8_counts) on the GPU.

The adaptive render is checked EXACTLY: in the static mode (slots_per_pixel=1) every round is the reference's per-pixel sum
over a sample range, so a numpy restatement of the rule in include/pt_amd.h over oracle renders of the same ranges reproduces
the sample counts and the sums bit for bit."""
import numpy as np
import pytest

from adaptive_rule import DeviceBuffer, adaptive_replay, bits, quantise_counts_np, schedule, sentinel_frame   # the rule, restated

pytestmark = pytest.mark.gpu


# ---- 1. all pixels listed ---------------------------------------------------------------------------------------------
def test_all_pixels_listed_equals_render(pt, ctx):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 60, 8)                       # 60 x 60: ragged 8x8 tiles at the right and bottom edges
    n = 60 * 60
    every = np.arange(n, dtype=np.uint32)
    ref, st = gs.render(cam, 5, 0, 8, slots_per_pixel=1)
    got, sp = gs.render_pixels(cam, 5, every, 0, 8, slots_per_pixel=1)
    np.testing.assert_array_equal(got, ref)
    assert sp.samples == st.samples == n * 8 and sp.segments == st.segments
    dref, dst = gs.render(cam, 5, 0, 8)
    dgot, dsp = gs.render_pixels(cam, 5, every, 0, 8)
    np.testing.assert_allclose(dgot, dref, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(dgot, ref, rtol=1e-13, atol=1e-13)
    assert dsp.samples == dst.samples == n * 8 and dsp.segments == dst.segments
    gs.close()


# ---- 2. a random subset -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 0])
def test_random_subset_writes_only_the_listed_pixels(pt, ctx, k):
    rng = np.random.default_rng(7 + k)
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 52, 6)
    h, w = 52, 52
    ref, _ = gs.render(cam, 2, 2, 6, slots_per_pixel=k)
    sel = np.sort(rng.choice(h * w, size=int(0.3 * h * w), replace=False)).astype(np.uint32)
    mask = np.zeros(h * w, dtype=bool)
    mask[sel] = True
    mask = mask.reshape(h, w)
    base = sentinel_frame((h, w, 3), rng)

    def check(out, overwrite):
        np.testing.assert_array_equal(bits(out[~mask]), bits(base[~mask]))          # unlisted: the sentinel, bit for bit
        want = ref[mask] if overwrite else base[mask] + ref[mask]
        if k == 1:
            np.testing.assert_array_equal(out[mask], want)
        else:
            np.testing.assert_allclose(out[mask], want, rtol=1e-13, atol=1e-13)

    for overwrite in (False, True):
        out, st = gs.render_pixels(cam, 2, sel, 2, 6, accum=base.copy(), slots_per_pixel=k, overwrite=overwrite)
        check(out, overwrite)
        assert st.samples == len(sel) * 4
        dev = DeviceBuffer(base.copy())
        gs.render_pixels(cam, 2, sel, 2, 6, slots_per_pixel=k, overwrite=overwrite, device_ptr=dev.ptr.value)
        check(dev.get(), overwrite)
        dev.free()
    # n == 0 is a no-op
    out, st = gs.render_pixels(cam, 2, np.zeros(0, np.uint32), 0, 6, accum=base.copy(), slots_per_pixel=k)
    np.testing.assert_array_equal(bits(out), bits(base))
    assert st.samples == 0
    gs.close()


def test_bad_pixel_lists_are_refused(pt, ctx):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 40, 4)
    base = np.full((40, 40, 3), 0.5)
    for bad, what in (([5, 3, 9], "ascending"), ([1, 4, 4, 7], "ascending"), ([0, 40 * 40], "range")):
        acc = base.copy()
        with pytest.raises(pt.PtError, match=what):
            gs.render_pixels(cam, 1, np.array(bad, np.uint32), 0, 4, accum=acc, slots_per_pixel=1)
        np.testing.assert_array_equal(acc, base)
    gs.close()


# ---- 3. adaptive, static mode: bit-exact against the oracle -----------------------------------------------------------
def test_adaptive_static_bit_exact_vs_oracle(pt, det, ctx):
    m, n, thr, seed = 4, 32, 0.5, 3
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 48, n)
    os_ = det.Scene()
    ocam = os_.build_scene(3, 48, n)
    acc, counts, st = gs.render_adaptive(cam, seed, m, n, thr, slots_per_pixel=1)
    want, want_counts, rounds = adaptive_replay(lambda lo, hi: os_.render(ocam, seed, lo, hi)[0], 48, 48, m, n, thr)
    stop_rounds = set(np.unique(rounds[rounds >= 0]).tolist())
    assert len(stop_rounds) >= 3, f"pixels stopped in rounds {sorted(stop_rounds)} only: pick another threshold"
    assert (want_counts == n).any()                                       # and some never stop
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(acc, want)
    assert st.samples == int(counts.sum())
    gs.close(); os_.close()


# ---- 4. threshold <= 0 is a uniform render ----------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.0, -1.0])
def test_adaptive_without_threshold_is_uniform(pt, ctx, thr):
    m, n, seed = 6, 40, 4
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 44, n)
    acc, counts, st = gs.render_adaptive(cam, seed, m, n, thr, slots_per_pixel=1)
    assert (counts == n).all() and st.samples == 44 * 44 * n
    every = np.arange(44 * 44, dtype=np.uint32)
    E, O = np.zeros_like(acc), np.zeros_like(acc)
    b = schedule(m, n)
    for i in range(len(b) - 1):
        gs.render_pixels(cam, seed, every, b[i], b[i + 1], accum=E if i % 2 == 0 else O, slots_per_pixel=1)
    np.testing.assert_array_equal(acc, E + O)
    plain, _ = gs.render(cam, seed, 0, n, slots_per_pixel=1)
    np.testing.assert_allclose(acc, plain, rtol=1e-12, atol=0)
    gs.close()


# ---- 5. dynamic against static ----------------------------------------------------------------------------------------
def test_adaptive_dynamic_agrees_with_static(pt, ctx):
    m, n, thr, seed = 8, 96, 0.05, 1
    gs = pt.Scene(ctx)
    cam = gs.build_scene(6, 320, n)
    sa, sc, sst = gs.render_adaptive(cam, seed, m, n, thr, slots_per_pixel=1)
    da, dc, dst = gs.render_adaptive(cam, seed, m, n, thr, slots_per_pixel=0)
    same = sc == dc
    assert same.mean() >= 0.999, f"spp maps agree on {same.mean():.5f} of the pixels"
    assert 0.0 < (sc < n).mean() < 1.0                                   # the threshold does something, and not everything
    np.testing.assert_allclose(da[same], sa[same], rtol=1e-12, atol=0)
    assert sst.samples == int(sc.sum()) and dst.samples == int(dc.sum())
    gs.close()


# ---- 6. resolve with per-pixel counts ---------------------------------------------------------------------------------
def test_resolve_u8_counts(pt, ctx):
    rng = np.random.default_rng(3)
    h, w, spp = 37, 29, 24
    acc = rng.uniform(0.0, 2.0 * spp, size=(h, w, 3))
    flat = acc.reshape(-1)
    flat[::17] = np.nan
    flat[1::19] = -1.0
    flat[2::23] = np.inf
    uniform = np.full((h, w), spp, dtype=np.uint32)
    np.testing.assert_array_equal(ctx.resolve_u8_counts(acc, uniform), ctx.resolve_u8(acc, spp))
    mixed = rng.integers(1, 4000, size=(h, w)).astype(np.uint32)
    np.testing.assert_array_equal(ctx.resolve_u8_counts(acc, mixed), quantise_counts_np(acc, mixed))
    with pytest.raises(pt.PtError, match="no samples"):
        ctx.resolve_u8_counts(acc, np.zeros((h, w), np.uint32))


# ---- 7. it saves samples without losing accuracy ----------------------------------------------------------------------
# Calibrated on one MI355X run (tools/adaptive_eval.py --calibrate, five seeds): see the docstring.
MEAN_SPP_FRACTION_MAX = 0.86
ERR_MULTIPLE_MAX = 0.35


def test_adaptive_saves_samples_and_keeps_accuracy(pt, ctx):
    """Scene 3 (Cornell box) at 128 px, min 16, max 1024, threshold 0.1, against an 8192-spp render.
    The true error of a pixel is the same statistic the rule estimates, taken against the reference mean:
    sum_c |mean_c - ref_c| / (1e-4 + sqrt(sum_c ref_c)).
    Measured on one MI355X run, seeds 1-5 (dynamic mode):
      mean spp / max_spp          0.8389 0.8407 0.8408 0.8421 0.8434   mean 0.8412  sigma 0.0017  -> bound 0.86 (11 sigma above)
      true error of the stopped
      pixels / threshold          0.2677 0.2613 0.2702 0.2567 0.2682   mean 0.2648  sigma 0.0057  -> bound 0.35 (15 sigma above)
    (the two-set estimate |A - B| is about twice the error of their mean, and a pixel stops only when its neighbours agree)."""
    m, n, thr = 16, 1024, 0.1
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, 128, n)
    ref, _ = gs.render(cam, 99, 0, 8192)
    ref = ref / 8192.0
    acc, counts, st = gs.render_adaptive(cam, 1, m, n, thr)
    mean = acc / counts[..., None].astype(np.float64)
    frac = counts.mean() / n
    stopped = counts < n
    true_err = np.abs(mean - ref).sum(axis=2) / (1e-4 + np.sqrt(ref.sum(axis=2)))
    ratio = true_err[stopped].mean() / thr
    print(f"adaptive scene 3 128px: mean spp fraction {frac:.4f}, stopped {stopped.mean():.4f}, true error / threshold {ratio:.4f}")
    assert frac < MEAN_SPP_FRACTION_MAX
    assert stopped.any()
    assert ratio < ERR_MULTIPLE_MAX
    gs.close()
