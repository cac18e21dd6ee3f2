"""Shading-order output of the dynamic mode (PoolD::reorder): k_shade writes every path to its position in the window's sorted
order in a second record area instead of back into the slot it came from. Which slot a path sits in decides nothing (the RNG is
keyed by pixel and sample, the accumulator by pixel), so the ordered frame must equal the in-place one (PT_POOL_IN_PLACE=1) up to
the order of the f64 atomics, on pools small enough to reach the frame's end, the compaction and the work-counter shards running
dry, and every sample must stay the oracle's, bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


@pytest.mark.parametrize("sid, width, spp", [(6, 96, 40), (3, 64, 24)])
def test_shading_order_equals_in_place(pt, ctx, sid, width, spp):
    gs = pt.Scene(ctx)
    cam = gs.build_scene(sid, width, spp)
    for pool in (None, "4096", "70000"):
        env = {"PT_EXPERIMENT": "1"}
        if pool: env["PT_POOL_SLOTS"] = pool
        ordered, st = _with_env(env, lambda: gs.render(cam, 3, 0, spp))
        in_place, st_ip = _with_env(dict(env, PT_POOL_IN_PLACE="1"), lambda: gs.render(cam, 3, 0, spp))
        assert st.samples == st_ip.samples == ordered.shape[0] * ordered.shape[1] * spp, (pool, st.samples, st_ip.samples)
        assert st.segments == st_ip.segments, (pool, st.segments, st_ip.segments)
        fin = np.isfinite(in_place)
        assert (np.isfinite(ordered) == fin).all(), pool
        np.testing.assert_allclose(ordered[fin], in_place[fin], rtol=1e-12, atol=0.0, err_msg=f"scene {sid} pool {pool}")
        if pool is None:
            assert st.compactions >= 1                 # one sample per slot: the frame is nothing but its end
    gs.close()


def test_shading_order_samples_bit_exact(pt, det, ctx, scene_images):
    """200 (pixel, sample) pairs of one-sample slices rendered in the dynamic mode on a 4096-slot pool (every slot regenerates
    camera rays several times, into the sorted positions of the output area) against the oracle's trace of that sample."""
    gs, os_ = pt.Scene(ctx), det.Scene()
    cam = gs.build_scene(6, 160, 200)
    ocam = os_.build_scene(6, 160, 200, images=scene_images(6))
    rng = np.random.default_rng(11)
    checked = 0
    for sample in (0, 7, 58, 191):
        acc, st = _with_env({"PT_EXPERIMENT": "1", "PT_POOL_SLOTS": "4096"}, lambda: gs.render(cam, 1, sample, sample + 1))
        assert st.samples == acc.shape[0] * acc.shape[1] and st.n_slots == 4096
        flat = acc.reshape(-1, 3)
        for pix in rng.integers(0, flat.shape[0], 50):
            rad, _, _ = os_.trace_sample(ocam, 1, int(pix), sample)
            np.testing.assert_array_equal(flat[pix], rad, err_msg=f"pixel {pix} sample {sample}")
            checked += 1
    assert checked == 200
    gs.close(); os_.close()
