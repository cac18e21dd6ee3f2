"""Adaptive sampling (pt_render_adaptive: the k_adapt_* kernels of csrc/pt_adaptive.hip), pt_resolve_u8_counts and pixel-list renders
(pt_render_pixels: the LIST forms of k_resolve / k_detile) at the frame shapes at which their index arithmetic takes another path:
ragged 8x8 tiles on either side, one tile row or column, one tile, one pixel; more than 1024 select blocks (k_adapt_scan serialises
per > 1 counts per thread); more pixels than the grid caps cover in one go (the grid-stride loops of k_adapt_error, k_adapt_final and
k_quantise_counts); odd, minimal and degenerate schedules and thresholds; isolated noisy pixels at the frame's corners, edges and tile
seams; lists of 1, 63, 64 and 65 pixels and a dynamic list render long enough for the end-of-frame pool compaction.

The static mode (slots_per_pixel=1) is checked EXACTLY against tests/adaptive_rule.py's replay of the rule, fed from the device's own
static whole-frame renders of the same sample ranges (bit-exact against the oracle: tests/test_gpu_parity.py; equal to the static list
render: test_all_pixels_listed_equals_render), and once from the oracle itself."""
import time

import numpy as np
import pytest

from adaptive_rule import DeviceBuffer, adaptive_replay, bits, dilate, error_estimate, quantise_counts_np, schedule, sentinel_frame, tiled_index
from common import SceneSpec, _with_env, default_camera, random_scene

pytestmark = pytest.mark.gpu

M, N, THR, SEED = 4, 32, 0.5, 3          # scene 3 at these stops pixels in many rounds and leaves some running (test_adaptive_gpu.py)


def _frame(pt, gs, scene, w, h, spp):
    cam = gs.build_scene(scene, w, spp)
    cam.aspect_ratio = w / (h + 0.5)
    assert pt.image_height(cam) == h
    return cam


def _device_ranges(gs, cam, seed):
    return lambda lo, hi: gs.render(cam, seed, lo, hi, slots_per_pixel=1)[0]


def _exact(ctx, gs, cam, w, h, m, n, thr, seed, render_range=None, min_rounds=3, some_never=True):
    """One static adaptive render against the replay: counts and sums array_equal, the sample total, the resolve. min_rounds / some_never:
    the guards of a general case — pixels stop in that many distinct rounds, and some never do."""
    acc, counts, st = gs.render_adaptive(cam, seed, m, n, thr, slots_per_pixel=1)
    want, want_counts, rounds = adaptive_replay(render_range or _device_ranges(gs, cam, seed), h, w, m, n, thr)
    stop_rounds = sorted(set(np.unique(rounds[rounds >= 0]).tolist()))
    print(f"{w}x{h} m {m} n {n} thr {thr}: stop rounds {stop_rounds}, never stopped {(rounds < 0).mean():.4f}, mean spp {want_counts.mean():.2f}")
    assert len(stop_rounds) >= min_rounds, f"pixels stopped in rounds {stop_rounds} only: pick another threshold"
    if some_never:
        assert (want_counts == n).any(), "every pixel stops early: pick another threshold"
    assert acc.shape == (h, w, 3) and counts.shape == (h, w)
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(acc, want)
    assert st.samples == int(counts.sum())
    np.testing.assert_array_equal(ctx.resolve_u8_counts(acc, counts), quantise_counts_np(acc, counts))
    return acc, counts, st, rounds


# ---- 2a. ragged frames --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w, h", [(60, 44), (44, 60), (5, 40), (40, 5), (8, 8)])
def test_ragged_frames_replay_exactly(pt, ctx, w, h):
    """Tiles ragged at the right (60, 44 = 5.5 tiles), at the bottom, on both sides; one tile column / one tile row of ragged tiles only
    (tiles_x == 1 / tiles_y == 1); exactly one whole tile."""
    gs = pt.Scene(ctx)
    cam = _frame(pt, gs, 3, w, h, N)
    _exact(ctx, gs, cam, w, h, M, N, THR, SEED)
    gs.close()


def test_ragged_frame_replays_exactly_from_the_oracle(pt, det, ctx):
    """60x44 once more with the replay fed by the oracle's renders, so that the chain does not rest on the device alone."""
    w, h = 60, 44
    gs = pt.Scene(ctx)
    cam = _frame(pt, gs, 3, w, h, N)
    os_ = det.Scene()
    ocam = os_.build_scene(3, w, N)
    ocam.aspect_ratio = w / (h + 0.5)
    assert det.image_height(ocam) == h
    _exact(ctx, gs, cam, w, h, M, N, THR, SEED, render_range=lambda lo, hi: os_.render(ocam, SEED, lo, hi)[0])
    gs.close(); os_.close()


# ---- 2b. more than 1024 select blocks -----------------------------------------------------------------------------------------------------
def test_more_than_1024_select_blocks(pt, ctx):
    """516x508: 65 x 64 tiles, 1040 blocks of 256 tiled indices, so every thread of k_adapt_scan's one block serialises per = 2 counts, the
    threads from 520 on have none (lo >= n_blocks), and both frame sides are ragged.
    Measured on one MI355X: 0.32 s, the scene's build and the replay's six renders included."""
    w, h = 516, 508
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    assert -(-tiles * 64 // 256) > 1024
    t0 = time.perf_counter()
    gs = pt.Scene(ctx)
    cam = _frame(pt, gs, 3, w, h, N)
    _, _, _, rounds = _exact(ctx, gs, cam, w, h, M, N, THR, SEED)
    survivors = tiled_index(h, w)[rounds != 1]                            # who goes on after the first test (round 1), in tiled order
    assert (survivors < tiles * 64 // 8).any() and (survivors >= tiles * 64 * 7 // 8).any(), "no survivor at one end: the scan's carry is not seen"
    gs.close()
    print(f"516x508: {time.perf_counter() - t0:.2f} s")


# ---- 2c. more than 2 097 152 pixels -------------------------------------------------------------------------------------------------------
def test_more_pixels_than_the_grid_caps_cover(pt, ctx):
    """1452x1446 = 2 099 592 pixels, min 4, max 12 (bounds 0 2 4 6 9 12: three tests): k_adapt_error and k_adapt_final (8192 blocks of 256
    threads) go round their grid-stride loops a second time, and the scan runs at per = 9 (8236 blocks). With three tests pixels can stop in
    three rounds at most, and they do: the guard stays at three.
    Measured on one MI355X: 0.76 s, the scene's build and the replay's five renders included."""
    w, h, m, n = 1452, 1446, 4, 12
    assert w * h > 8192 * 256 and schedule(m, n) == [0, 2, 4, 6, 9, 12]
    t0 = time.perf_counter()
    gs = pt.Scene(ctx)
    cam = _frame(pt, gs, 3, w, h, n)
    _exact(ctx, gs, cam, w, h, m, n, THR, SEED)
    gs.close()
    print(f"1452x1446: {time.perf_counter() - t0:.2f} s")


# ---- 2d. schedules ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m, n, tests", [(5, 40, 6), (2, 9, 4), (6, 7, 1), (8, 8, 0)])
def test_schedules(pt, ctx, m, n, tests):
    """(5, 40): bounds 0 2 5 ..., so n_E = 2 and n_O = 3 at the first test; (2, 9): one-sample rounds; (6, 7): one test; (8, 8): none.
    With t tests pixels can stop in at most t distinct rounds: the guard asks for min(t, 3)."""
    w, h = 60, 44
    b = schedule(m, n)
    assert sum(1 for i in range(1, len(b) - 1) if b[i + 1] < n) == tests
    gs = pt.Scene(ctx)
    cam = _frame(pt, gs, 3, w, h, n)
    acc, counts, st, _ = _exact(ctx, gs, cam, w, h, m, n, THR, SEED, min_rounds=min(tests, 3))
    if tests == 0:
        assert (counts == n).all() and st.samples == w * h * n
        rr = _device_ranges(gs, cam, SEED)
        np.testing.assert_array_equal(acc, rr(0, m // 2) + rr(m // 2, m))
    gs.close()


# ---- 2e. degenerate thresholds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [1e30, np.inf, np.nan])
def test_degenerate_thresholds(pt, ctx, thr):
    """1e30 and inf: every pixel with finite sums stops at the first test (n_active == 0: the scan of all zeros, the early end of the round
    loop); NaN: no comparison with it holds, so nobody stops, as for a threshold <= 0."""
    w, h = 60, 44
    gs = pt.Scene(ctx)
    cam = _frame(pt, gs, 3, w, h, N)
    acc, counts, st, _ = _exact(ctx, gs, cam, w, h, M, N, thr, SEED, min_rounds=0 if thr != thr else 1, some_never=False)
    rr = _device_ranges(gs, cam, SEED)
    if thr != thr:
        assert (counts == N).all() and st.samples == w * h * N
    else:
        first = rr(0, M // 2) + rr(M // 2, M)
        finite = np.isfinite(first).all(axis=2)
        assert (counts[finite] == M).all()
        np.testing.assert_array_equal(acc[finite], first[finite])
        if finite.all():
            np.testing.assert_array_equal(acc, first)
            assert st.samples == w * h * M
    gs.close()


# ---- 2f. non-finite pixels never stop -----------------------------------------------------------------------------------------------------
def test_non_finite_pixels_never_stop_scene_6(pt, ctx):
    """Scene 6 at 96x54: wherever a pixel's sums are not finite, it and its eight neighbours must have run to the end. On the oracle this
    frame has no such pixel at these parameters, nor with seeds 1 to 12 and up to 1024 samples, so here the condition holds vacuously and
    the case is the exact replay on a second scene; test_non_finite_pixels_never_stop has a scene that does produce them."""
    w, h = 96, 54
    gs = pt.Scene(ctx)
    cam = gs.build_scene(6, w, N)
    assert pt.image_height(cam) == h
    acc, counts, _, _ = _exact(ctx, gs, cam, w, h, M, N, THR, SEED)
    broken = ~np.isfinite(acc).all(axis=2)
    print(f"scene 6 {w}x{h}: {int(broken.sum())} pixels with non-finite sums")
    assert (counts[dilate(broken)] == N).all()
    gs.close()


def test_non_finite_pixels_never_stop(pt, ctx):
    """A scene whose own estimator yields NaN: a sphere in the lights list (the reference's Sphere::pdf is NaN for origins on the sphere,
    tests/common.py random_scene), at 52x37. A pixel whose sums are not finite never stops, whenever that happened; its neighbours never
    stop if it was already so at the first test (a neighbour may have stopped before a later sample broke the pixel)."""
    w, h = 52, 37
    spec, gs = random_scene(1, with_mesh=False, sphere_light=True), pt.Scene(ctx)
    spec.camera.update(image_width=w, aspect_ratio=w / (h + 0.5))
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    assert pt.image_height(cam) == h
    rr = _device_ranges(gs, cam, SEED)
    acc, counts, _, _ = _exact(ctx, gs, cam, w, h, M, N, THR, SEED, render_range=rr)
    broken = ~np.isfinite(acc).all(axis=2)
    early = ~np.isfinite(rr(0, M // 2) + rr(M // 2, M)).all(axis=2)
    print(f"sphere-light scene {w}x{h}: {int(broken.sum())} pixels with non-finite sums, {int(early.sum())} of them at the first test")
    assert early.sum() >= 10 and (broken & ~early).any() and (~dilate(broken)).sum() >= 100, "pick another scene seed"
    assert (counts[broken] == N).all() and (counts[dilate(early)] == N).all()
    assert (counts[~dilate(broken)] < N).any()                            # ... and the rule still stops pixels elsewhere
    gs.close()


# ---- 2g. dilation at the frame's corners and edges and across a tile seam -----------------------------------------------------------------
EDGE_M, EDGE_N, EDGE_THR = 4, 24, 0.05


def _edge_scene(pt, w, h, pixels):
    """A constant grey environment (0.25: every sum of it is exact, so a pixel that sees nothing else has error 0 exactly), no lights, a pinhole
    camera, and on the camera ray of each of `pixels` (y, x) a small diffuse sphere under a fine 0.9 / 0.05 checker, centred in the focal plane
    on the pixel's centre with a radius of 0.4 pixels: the pixel's samples (a disc of 0.5 pixels) hit or miss it and land on either colour,
    and no other pixel's sample can reach it."""
    camera = default_camera(width=w, aspect=w / (h + 0.5), spp=EDGE_N, defocus_angle=0.0, env_is_map=0, env_color=(0.25, 0.25, 0.25))
    probe = SceneSpec()
    probe.camera = camera
    v, height = pt.camera_init(probe.make_camera(pt.Camera, []))
    assert height == h
    r = 0.4 * float(np.linalg.norm(v["pixel_du"]))
    s = SceneSpec()
    mat = s.add("mat_diffuse", s.add("tex_checker", r / 3.0, s.add("tex_solid_rgb", 0.9, 0.9, 0.9), s.add("tex_solid_rgb", 0.05, 0.05, 0.05)), -1)
    for y, x in pixels:
        c = tuple(float(a) for a in v["pixel00"] + x * v["pixel_du"] + y * v["pixel_dv"])
        s.add("world_add_object", s.add("sphere", r, c, c, mat))
    s.add("world_build")
    s.camera = camera
    return s


# frame -> seed, the pixels (y, x) with a sphere, and the (seam pixel, its neighbour across the tile seam) pairs among them
EDGE_CASES = {
    (21, 13): (20, [(0, 0), (12, 20), (0, 10), (12, 10), (6, 0), (6, 20), (3, 7), (7, 14)], [((3, 7), (3, 8)), ((7, 14), (8, 14))]),
    (5, 40): (25, [(0, 0), (39, 4), (0, 2), (39, 2), (13, 0), (26, 4), (7, 2)], [((7, 2), (8, 2))]),
}


@pytest.mark.parametrize("w, h", sorted(EDGE_CASES))
def test_dilation_at_corners_edges_and_tile_seams(pt, ctx, w, h):
    seed, pixels, seams = EDGE_CASES[(w, h)]
    spec, gs = _edge_scene(pt, w, h, pixels), pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    rr = _device_ranges(gs, cam, seed)
    _, counts, _, rounds = _exact(ctx, gs, cam, w, h, EDGE_M, EDGE_N, EDGE_THR, seed, render_range=rr, min_rounds=1, some_never=False)
    bad = ~(error_estimate(rr(0, 2), rr(2, 4), 2, 2) < EDGE_THR)         # the first test, as the replay ran it
    for y, x in pixels:
        assert bad[y, x], f"pixel ({y}, {x}) is not noisy at the first test: pick another seed"
    for _, (y, x) in seams:
        assert not bad[y, x] and counts[y, x] > EDGE_M                    # kept across the seam though not bad itself
    kept = dilate(bad)
    np.testing.assert_array_equal(rounds != 1, kept)
    assert bad.sum() == len(pixels) and kept.sum() < w * h / 2
    assert (counts[~kept] == EDGE_M).all()                                # farther than one pixel from every bad one: stopped at once
    gs.close()


def test_one_pixel_frame(pt, ctx):
    """1x1: one ragged tile, one select block, 63 tiled indices outside the frame."""
    spec, gs = _edge_scene(pt, 1, 1, [(0, 0)]), pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    _, counts, _, _ = _exact(ctx, gs, cam, 1, 1, EDGE_M, EDGE_N, EDGE_THR, 1, min_rounds=0, some_never=False)
    assert counts[0, 0] > EDGE_M
    gs.close()


# ---- 3a. a dynamic list render that compacts its pool -------------------------------------------------------------------------------------
def test_dynamic_list_render_compacts_its_pool(pt, ctx):
    """Scene 3 at 250x210, a random 80 % of the pixels, samples [0, 3): 126 000 slots, which die as the work runs out, so the end-of-frame
    compaction (k_compact_scan / k_compact_move, n_alloc > 4 * 8192) runs under a pixel list and k_detile's LIST form reads what it left.
    1e-11: test_end_of_frame_pool_compaction_changes_no_result's bound for the same comparison."""
    rng = np.random.default_rng(11)
    w, h, seed = 250, 210, 6
    gs = pt.Scene(ctx)
    cam = _frame(pt, gs, 3, w, h, 3)
    sel = np.sort(rng.choice(h * w, size=int(0.8 * h * w), replace=False)).astype(np.uint32)
    mask = np.zeros(h * w, dtype=bool)
    mask[sel] = True
    mask = mask.reshape(h, w)
    base = sentinel_frame((h, w, 3), rng)
    ref, rst = gs.render_pixels(cam, seed, sel, 0, 3, slots_per_pixel=1)
    assert rst.samples == len(sel) * 3 and (ref[~mask] == 0.0).all()
    want = base + ref
    finite = np.isfinite(want) & mask[..., None]

    def check(out, st):
        np.testing.assert_array_equal(bits(out[~mask]), bits(base[~mask]))          # unlisted: the sentinel, bit for bit
        np.testing.assert_allclose(out[finite], want[finite], rtol=1e-11, atol=1e-11)
        np.testing.assert_array_equal(np.isfinite(out), np.isfinite(want))
        assert st.samples == rst.samples and st.segments == rst.segments
        return st.compactions

    def both(env):
        run = (lambda f: _with_env(env, f)) if env else (lambda f: f())
        out, st = run(lambda: gs.render_pixels(cam, seed, sel, 0, 3, accum=base.copy()))
        n_host = check(out, st)
        dev = DeviceBuffer(base.copy())
        _, st = run(lambda: gs.render_pixels(cam, seed, sel, 0, 3, device_ptr=dev.ptr.value))
        out = dev.get()
        dev.free()
        return n_host, check(out, st)

    made = both(None)
    print(f"list render {w}x{h}, {len(sel)} pixels: compactions {made}")
    assert min(made) >= 1
    assert both({"PT_EXPERIMENT": "1", "PT_NO_COMPACT_POOL": "1"}) == (0, 0)
    for switch in ({"PT_COMPACT_AT": "85"}, {"PT_POLL_CAP": "1"}):
        print(f"  {switch}: compactions {both(dict(switch, PT_EXPERIMENT='1'))}")
    gs.close()


# ---- 3b. the adaptive driver over the same machinery --------------------------------------------------------------------------------------
def test_adaptive_dynamic_with_degenerate_thresholds_is_a_plain_render(pt, ctx):
    """The dynamic mode's counts are deterministic where the threshold decides for every pixel alike: 0 stops nobody, 1e30 everybody."""
    w, h, m, n, seed = 250, 210, 4, 32, 3
    gs = pt.Scene(ctx)
    cam = _frame(pt, gs, 3, w, h, n)
    for thr, spp in ((0.0, n), (1e30, m)):
        plain, pst = gs.render(cam, seed, 0, spp, slots_per_pixel=1)
        assert np.isfinite(plain).all()
        acc, counts, st = gs.render_adaptive(cam, seed, m, n, thr)
        assert (counts == spp).all()
        np.testing.assert_allclose(acc, plain, rtol=1e-11, atol=1e-11)
        assert st.samples == pst.samples == w * h * spp and st.segments == pst.segments
        print(f"adaptive dynamic {w}x{h} thr {thr}: compactions {st.compactions}")
    gs.close()


# ---- 3c. list lengths around the 64-item work run -----------------------------------------------------------------------------------------
def _lists(w, h):
    order = np.argsort(tiled_index(h, w).reshape(-1), kind="stable")      # the pixels in tiled order
    y, x = np.mgrid[h - h % 8:h, w - w % 8:w]
    lists = {"first pixel": [0], "last pixel": [w * h - 1], "ragged corner tile": (y * w + x).reshape(-1), "all but one": np.delete(np.arange(w * h), 1234)}
    lists.update({f"first {k} in tiled order": order[:k] for k in (63, 64, 65)})
    return {name: np.sort(np.asarray(v)).astype(np.uint32) for name, v in lists.items()}


@pytest.mark.parametrize("k", [1, 0])
def test_list_lengths(pt, ctx, k):
    """Scene 3 at 60x60 (tiles ragged on both sides; the corner tile holds 4x4 pixels), samples [2, 6). Static: equal to the whole-frame
    render; dynamic: 1e-13, test_random_subset_writes_only_the_listed_pixels' bound."""
    rng = np.random.default_rng(5)
    w = h = 60
    gs = pt.Scene(ctx)
    cam = gs.build_scene(3, w, 6)
    assert pt.image_height(cam) == h
    ref, _ = gs.render(cam, 2, 2, 6, slots_per_pixel=1)
    base = sentinel_frame((h, w, 3), rng)
    lists = _lists(w, h)
    assert [len(v) for v in lists.values()] == [1, 1, 16, w * h - 1, 63, 64, 65]
    for name, sel in lists.items():
        mask = np.zeros(h * w, dtype=bool)
        mask[sel] = True
        mask = mask.reshape(h, w)
        dev = DeviceBuffer(base.copy())
        out, st = gs.render_pixels(cam, 2, sel, 2, 6, accum=base.copy(), slots_per_pixel=k)
        _, sd = gs.render_pixels(cam, 2, sel, 2, 6, slots_per_pixel=k, device_ptr=dev.ptr.value)
        for got, stats in ((out, st), (dev.get(), sd)):
            np.testing.assert_array_equal(bits(got[~mask]), bits(base[~mask]), err_msg=name)
            if k == 1:
                np.testing.assert_array_equal(got[mask], base[mask] + ref[mask], err_msg=name)
            else:
                np.testing.assert_allclose(got[mask], base[mask] + ref[mask], rtol=1e-13, atol=1e-13, err_msg=name)
            assert stats.samples == len(sel) * 4, name
        dev.free()
    gs.close()


# ---- 4. pt_resolve_u8_counts above its grid cap -------------------------------------------------------------------------------------------
def test_resolve_u8_counts_above_its_grid_cap(pt, ctx):
    """1100x960 = 1 056 000 pixels: k_quantise_counts (at most 4096 blocks of 256 threads) goes round its grid-stride loop a second time."""
    rng = np.random.default_rng(3)
    h, w, spp = 960, 1100, 24
    assert h * w > 4096 * 256
    acc = rng.uniform(0.0, 2.0 * spp, size=(h, w, 3))
    flat = acc.reshape(-1)
    flat[::17] = np.nan
    flat[1::19] = -1.0
    flat[2::23] = np.inf
    mixed = rng.integers(1, 4000, size=(h, w)).astype(np.uint32)
    np.testing.assert_array_equal(ctx.resolve_u8_counts(acc, mixed), quantise_counts_np(acc, mixed))
    uniform = np.full((h, w), spp, dtype=np.uint32)
    np.testing.assert_array_equal(ctx.resolve_u8_counts(acc, uniform), ctx.resolve_u8(acc, spp))
