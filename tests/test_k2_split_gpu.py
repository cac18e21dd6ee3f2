"""K2's mid-window rounds (csrc/pt_k2_extend.h "rounds of a window"). A full window of k_extend2 whose first half has filled
more than half of the candidate list runs phase B there and again at its end (the default, PT_K2_SPLIT=1); PT_K2_SPLIT=0 is the kernel
without the rule, PT_K2_SPLIT=2 the drain form. None of them may change a hit word, and the statistics k2_split_windows /
k2_overflow_rays say which path ran.

With the product grid (2048 blocks) every window of a pool under 2 M slots is a tail window, which never splits: the cases run K2 on four
blocks (PT_K2_BLOCKS=4) over a pool of 16384 slots — sixteen 1024-slot windows of the 128-thread form, twelve full and four tail — at
128x64 pixels and 16 samples per pixel.

What "equal" is. Sample and segment counts are equal, always. A frame of several samples per pixel is a sum of f64 atomic adds whose order
changes from run to run: two renders of one frame with the same switches differ in the last bits (measured on these scenes: up to
5.3e-15 absolute), so np.array_equal on a 16-sample render compares nothing but that order — such frames are held to the suite's bound for
reordered f64 adds, 1e-12 relative (tests/test_short_pass_gpu.py). Bit for bit — np.array_equal on the f64 sums — the frames are compared
as the suite does it everywhere: as sixteen one-sample renders summed on the host (tests/test_sky_pass_gpu.py _slices), where every pixel
receives one value per render. Those renders run with the sky and short-path passes off: K2 walks the pool from its end, and with the
passes on the 4096 samples of a one-sample render of this frame would lie in the four tail windows alone."""
import numpy as np
import pytest

from common import SceneSpec, _with_env, default_camera

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 128, 64, 16, 5
X = {"PT_EXPERIMENT": "1"}
GRID = dict(X, PT_K2_BLOCKS="4", PT_POOL_SLOTS="16384")
OFF, DRAIN, PRODUCT = dict(GRID, PT_K2_SPLIT="0"), dict(GRID, PT_K2_SPLIT="2"), dict(X, PT_POOL_SLOTS="16384")
NO_PASSES = dict(PT_SKY_PASS="0", PT_SHORT_PASS="0")
CAMERA = dict(width=W, aspect=W / (H + 0.5), spp=SPP, env_color=(0.6, 0.7, 0.9))
_SPOT = {}


def _spec(pt, mesh="left"):
    """A checker floor, a diffuse sphere on the right and assets/spot.obj under an instance, turned side on: scaled to fill the frame's left
    half ("left"); three smaller ones in a row along the frame's lower half ("low"); or none (None). Right is the camera's own."""
    s = SceneSpec()
    s.camera = default_camera(**CAMERA)
    frame, h = pt.camera_init(s.make_camera(pt.Camera, []))
    assert h == H
    right = frame["right"] / np.linalg.norm(frame["right"])
    floor = s.add("mat_diffuse", s.add("tex_checker", 0.8, s.add("tex_solid_rgb", 0.2, 0.3, 0.1), s.add("tex_solid_rgb", 0.9, 0.9, 0.9)), -1)
    red = s.add("mat_diffuse", s.add("tex_solid_rgb", 0.8, 0.3, 0.2), -1)
    grey = s.add("mat_diffuse", s.add("tex_solid_rgb", 0.7, 0.7, 0.7), -1)
    s.add("world_add_object", s.add("quad", (-30.0, -2.0, -30.0), (0.0, 0.0, 60.0), (60.0, 0.0, 0.0), floor))
    s.add("world_add_object", s.add("sphere", 1.2, tuple(2.8 * right + (0.0, 0.2, 0.0)), tuple(2.8 * right + (0.0, 0.2, 0.0)), red))
    if mesh is not None:
        if not _SPOT:
            _SPOT["P"], _SPOT["I"], _ = pt.load_obj(pt.ASSET_DIR + "/spot.obj")
        obj = s.add("mesh", 3.0 if mesh == "left" else 1.5, _SPOT["P"], _SPOT["I"], None, None, grey)
        for at in ([-2.8 * right + (0.0, 0.4, 0.0)] if mesh == "left" else [2.0 * k * right + (0.0, -0.9, -1.0) for k in (-1.5, 0.0, 1.5)]):
            s.add("world_add_object", s.add("instance", obj, (0.0, 1.0, 0.0), np.pi / 2.0, tuple(at)))
    s.add("world_build")
    return s


def _built(pt, ctx, mesh="left"):
    spec, gs = _spec(pt, mesh), pt.Scene(ctx)
    cam = spec.make_camera(pt.Camera, spec.replay(gs))
    assert pt.image_height(cam) == H
    return spec, gs, cam


def _render(gs, cam, env, a=0, b=SPP):
    return _with_env(env, lambda: gs.render(cam, SEED, a, b))


def _slices(gs, cam, env, n=SPP):
    """The frame as n one-sample renders summed on the host, the passes off; the statistics' counts added up."""
    acc, tot = None, dict(samples=0, segments=0, split=0, over=0)
    for i in range(n):
        a, st = _render(gs, cam, dict(env, **NO_PASSES), i, i + 1)
        acc = a if acc is None else acc + a
        for k, f in (("samples", "samples"), ("segments", "segments"), ("split", "k2_split_windows"), ("over", "k2_overflow_rays")):
            tot[k] += getattr(st, f)
    return acc, tot


def _same_frame(a, b):
    """Two 16-sample renders: counts equal, sums equal up to the order of their f64 adds (the module's docstring)."""
    (fa, sa), (fb, sb) = a, b
    assert sa.samples == sb.samples == W * H * SPP and sa.segments == sb.segments
    print(f"  max |difference| of the 16-sample frames {np.abs(fa - fb).max():.3e}")
    np.testing.assert_allclose(fa, fb, rtol=1e-12, atol=0.0)


def _same_bits(a, b):
    (fa, ta), (fb, tb) = a, b
    assert ta["samples"] == tb["samples"] == W * H * SPP and ta["segments"] == tb["segments"]
    assert np.array_equal(fa, fb)


@pytest.fixture(scope="module")
def shared(pt, ctx):
    """The mesh scene, and its frame under the default, the switch at 0 and the drain form: as one 16-sample render each and as one-sample
    slices — rendered once for every test that needs them."""
    spec, gs, cam = _built(pt, ctx)
    out = dict(spec=spec, gs=gs, cam=cam)
    for name, env in (("on", GRID), ("off", OFF), ("drain", DRAIN)):
        out[name], out[name + "_slices"] = _render(gs, cam, env), _slices(gs, cam, env)
        st, tot = out[name][1], out[name + "_slices"][1]
        print(f"{name}: K2 blocks {st.blocks_extend}, variant {st.extend_variant}, launches {st.launches_extend}, split windows {st.k2_split_windows}, "
              f"overflow rays {st.k2_overflow_rays}, segments {st.segments}; slices: split windows {tot['split']}, overflow rays {tot['over']}")
    yield out
    gs.close()


def test_default_against_the_switch_off_and_the_drain_form(shared):
    on, off, drain = shared["on"], shared["off"], shared["drain"]
    assert on[1].extend_variant == 0 and on[1].blocks_extend == off[1].blocks_extend == drain[1].blocks_extend == 4
    _same_frame(on, off)
    _same_frame(on, drain)
    _same_bits(shared["on_slices"], shared["off_slices"])
    _same_bits(shared["on_slices"], shared["drain_slices"])
    assert on[1].k2_split_windows > 0 and off[1].k2_split_windows == 0 and drain[1].k2_split_windows > 0
    assert off[1].k2_overflow_rays > 0 and on[1].k2_overflow_rays < off[1].k2_overflow_rays
    assert drain[1].k2_overflow_rays == 0                            # 128 threads: a tail round is CAND slots, a drained full window never runs out
    assert shared["on_slices"][1]["split"] > 0 and shared["off_slices"][1]["split"] == 0   # (the slices ran the rule too)


def test_the_product_grid_has_tail_windows_only(shared):
    """Without PT_K2_BLOCKS the grid is one block per window at most: every window of this pool is a tail window and none splits."""
    gs, cam = shared["gs"], shared["cam"]
    prod, prod_slices = _render(gs, cam, PRODUCT), _slices(gs, cam, PRODUCT)
    print(f"product grid: K2 blocks {prod[1].blocks_extend}, split windows {prod[1].k2_split_windows}, overflow rays {prod[1].k2_overflow_rays}")
    assert prod[1].blocks_extend > 16 and prod[1].k2_split_windows == 0 and prod[1].k2_overflow_rays == 0   # (a half window is CAND slots)
    assert prod_slices[1]["split"] == 0
    _same_frame(prod, shared["on"])
    _same_bits(prod_slices, shared["on_slices"])


def test_every_sample_is_the_oracles(shared, det):
    """Eight one-sample slices of the frame, every pixel bit-equal to the oracle's trace_sample in deterministic-math mode."""
    spec, gs, cam = shared["spec"], shared["gs"], shared["cam"]
    os_ = det.Scene()
    ocam = spec.make_camera(det.Camera, spec.replay(os_))
    split = 0
    for i in range(8):
        acc, st = _render(gs, cam, dict(GRID, **NO_PASSES), i, i + 1)
        split += st.k2_split_windows
        ref = np.array([os_.trace_sample(ocam, SEED, p, i, 1)[0] for p in range(H * W)]).reshape(H, W, 3)
        bad = np.argwhere((acc.view(np.uint64) != ref.view(np.uint64)).any(axis=2))
        assert len(bad) == 0, (i, bad[:4])
    print(f"samples compared {8 * H * W}, windows split {split}")
    assert split > 0
    os_.close()


def test_a_window_that_must_not_split_still_overflows(pt, ctx):
    """Meshes along the lower half of the frame. In the 128-thread form a split window cannot overflow (each of its rounds is at most CAND
    slots) and neither can a tail round, so every overflow ray counted under the default is of a full window the rule left alone: its
    first half at or below half the list, its second half over the rest. Phase A then walks those rays itself, the kernel's old path."""
    _, gs, cam = _built(pt, ctx, "low")
    on, off = _render(gs, cam, GRID), _render(gs, cam, OFF)
    print(f"low meshes: default split windows {on[1].k2_split_windows}, overflow rays {on[1].k2_overflow_rays}; switch at 0: overflow rays {off[1].k2_overflow_rays}")
    assert on[1].extend_variant == 0 and on[1].k2_split_windows > 0 and 0 < on[1].k2_overflow_rays < off[1].k2_overflow_rays
    _same_frame(on, off)
    _same_bits(_slices(gs, cam, GRID), _slices(gs, cam, OFF))
    gs.close()


def test_no_mesh_runs_the_batch_kernel(pt, ctx):
    _, gs, cam = _built(pt, ctx, None)
    on, off = _render(gs, cam, GRID), _render(gs, cam, OFF)
    assert on[1].extend_variant == 1
    for st in (on[1], off[1]):
        assert st.k2_split_windows == 0 and st.k2_overflow_rays == 0
    _same_frame(on, off)
    _same_bits(_slices(gs, cam, GRID), _slices(gs, cam, OFF))
    gs.close()


def test_the_deep_stack_form(shared):
    """PT_EXT2=204: 256 threads, 2048-slot windows (eight of this pool: four full, four tail), a list of 768. The rule only makes overflow
    rarer there — and a tail round, 1024 slots, can still run out of list under every switch."""
    gs, cam = shared["gs"], shared["cam"]
    deep = {k: _render(gs, cam, dict(env, PT_EXT2="204")) for k, env in (("on", GRID), ("off", OFF), ("drain", DRAIN))}
    for k, (_, st) in deep.items():
        print(f"deep {k}: split windows {st.k2_split_windows}, overflow rays {st.k2_overflow_rays}")
        _same_frame(deep[k], shared["on"])
    assert deep["off"][1].k2_split_windows == 0 and deep["on"][1].k2_split_windows > 0 and deep["drain"][1].k2_split_windows > 0
    assert deep["drain"][1].k2_overflow_rays < deep["on"][1].k2_overflow_rays < deep["off"][1].k2_overflow_rays
    _same_bits(_slices(gs, cam, dict(GRID, PT_EXT2="204")), shared["on_slices"])
    _same_bits(_slices(gs, cam, dict(DRAIN, PT_EXT2="204")), shared["on_slices"])


def test_the_tree_top_level(pt, ctx):
    """PT_NO_FLAT_TLAS=1 (read at the world's build): phase A walks the top-level tree with each lane's own stack."""
    _, gs, cam = _with_env(dict(X, PT_NO_FLAT_TLAS="1"), lambda: _built(pt, ctx))
    on, off = _render(gs, cam, GRID), _render(gs, cam, OFF)
    print(f"tree top level: split windows {on[1].k2_split_windows}, overflow rays {on[1].k2_overflow_rays} / {off[1].k2_overflow_rays} with the switch at 0")
    assert on[1].k2_split_windows > 0 and off[1].k2_split_windows == 0 and on[1].k2_overflow_rays < off[1].k2_overflow_rays
    _same_frame(on, off)
    _same_bits(_slices(gs, cam, GRID), _slices(gs, cam, OFF))
    gs.close()
