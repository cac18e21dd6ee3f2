"""Every compiled form of k_shade (csrc/pt_forms.h) launched on one scene, pinned to the others and to the oracle.

k_shade is one template compiled into 114 kernels: the shapes 22 and 32 (4096- and 8192-slot windows) x seven shading modes x lights
list or none x pixel list or whole frame x independent or Sobol sampler (LSE only with a lights list: 104 forms), and the legacy shapes
2, 3, 12, 13 and 52 in the PLAIN mode with and without a lights list (10 forms). A render picks the 8192-slot shape only on a pool of
at least 16 such windows per block launched, so a small test gets the 4096-slot shape unless it forces another one
(PT_EXPERIMENT=1 PT_SHADE_VARIANT=...). Here every form is forced in turn on common.forms_scene: 160 x 120 pixels, 19 200 slots in static
mode, 24 576 allocated — three 8192-slot windows or six 4096-slot windows, the last partly live in both — with many material classes
in every window.

One test per (mode, lights) x sampler, 26 in all, 4 spp and one seed. `ref` is the static (slots_per_pixel=1), whole-frame render at
shape 22. Each test checks:
  1. the form table: under every forced variant of {2, 3, 12, 13, 22, 32, 52}, whole frame and pixel list, the render reports the forced
     code exactly when the Python mirror of shade_form_exists says that form exists, and 42 (the fall-back) otherwise;
  2. static, whole frame: shape 32 — and for PLAIN with the independent sampler the five legacy shapes — equal ref bit for bit;
  3. static pixel lists of 1, 100 and 11 500 pixels (16 384 allocated slots: two 8192-slot windows, the second partly live) at shapes 22
     and 32: listed pixels equal ref bit for bit, the others keep the sentinel;
  4. dynamic mode at shapes 22 and 32, on the default pool and on 20 000 slots (work items are dequeued, shards stolen from, slots
     regenerate): whole frame, whole frame in place and the 11 500-pixel list agree with ref within rtol = atol = 1e-11 (at most spp f64
     additions in another order: the bound of the feature suites), with equal sample and segment counts;
  5. adaptive sampling (the production path of the list forms) gives identical sums and counts at shapes 22 and 32, with a threshold
     at which some pixels stop early and some never do;
  6. K2: ref rendered with the batch kernel instead of the two-phase one equals ref bit for bit;
  7. the anchor: for PLAIN with the independent sampler, ref and its segment count equal the deterministic-math oracle's render of the
     same SceneSpec bit for bit.
The other modes are anchored through a chain: each feature suite (test_env_sampling_gpu.py, test_medium_gpu.py, test_medium_grid_gpu.py,
test_interior_gpu.py, test_light_sampling_gpu.py, test_dispersion_gpu.py, test_sampler_gpu.py) pins its mode's 4096-slot whole-frame
form to a Python restatement of its rule, and this file pins every other form of that mode to that one.

The scene must keep every mode's code running: at least 99 % of every reference frame is finite, and every non-PLAIN frame differs from
the PLAIN frame of the same lights and sampler in at least a tenth of its pixels. Both are asserted."""
import os
import re

import numpy as np
import pytest

from common import FORMS_H, FORMS_MODES, FORMS_W, _with_env, forms_scene, window_slots

pytestmark = pytest.mark.gpu

SEED, SPP = 7, 4
N_PIXELS = FORMS_W * FORMS_H
LEGACY = (2, 3, 12, 13, 52)      # the shapes that exist in PLAIN only, whole frame, independent sampler; 22 and 32 have every form
LIST_SIZES = (1, 100, 11500)


def shade_form_exists(variant, lights, pixel_list, qmc, mode):
    """csrc/pt_forms.h shade_form_exists, restated."""
    return (variant in (22, 32, 42) or not (pixel_list or qmc or mode != "PLAIN")) and (mode != "LSE" or lights)


def shade_modes():
    """The names of ShadeMode in csrc/pt_types.h: a mode that common.forms_scene does not know would run in no test here."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "thu-acg-f2024-path-tracer_amd", "csrc", "pt_types.h")).read()
    return tuple(re.findall(r"MODE_(\w+)", re.search(r"enum ShadeMode \{([^}]*)\}", src).group(1)))


assert shade_modes() == FORMS_MODES, "add the new ShadeMode to common.forms_scene and FORMS_MODES"
CASES = [(m, l) for m in FORMS_MODES for l in (True, False) if shade_form_exists(22, l, False, False, m)]
assert len(CASES) == 13
LAUNCHED = set()      # (shape, lights, list, qmc, mode) of every k_shade form a render here reported: 114 after the whole file


def forced(variant, fn, **more):
    return _with_env(dict({"PT_EXPERIMENT": "1", "PT_SHADE_VARIANT": str(variant)}, **more), fn)


def pixel_list(n):
    return np.sort(np.random.default_rng(1000 + n).choice(N_PIXELS, size=n, replace=False)).astype(np.uint32)


def mask_of(sel):
    m = np.zeros(N_PIXELS, dtype=bool)
    m[sel] = True
    return m.reshape(FORMS_H, FORMS_W)


SENTINEL = np.random.default_rng(5).uniform(-3.0, 3.0, size=(FORMS_H, FORMS_W, 3))
SENTINEL.reshape(-1)[3::11] = np.nan
SENTINEL.flags.writeable = False


def same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def scenes(pt, ctx):
    """(mode, lights) -> (scene, camera, spec), built once."""
    built = {}

    def get(mode, lights):
        if (mode, lights) not in built:
            spec = forms_scene(mode, lights)
            gs = pt.Scene(ctx)
            built[mode, lights] = (gs, spec.make_camera(pt.Camera, spec.replay(gs)), spec)
        return built[mode, lights]

    yield get
    for gs, _, _ in built.values():
        gs.close()


REFS = {}


def reference(scenes, mode, lights, sampler):
    """The static whole-frame render at shape 22 and its stats, rendered once and read-only."""
    key = (mode, lights, sampler)
    if key not in REFS:
        gs, cam, _ = scenes(mode, lights)
        gs.set_sampler(sampler)
        ref, st = forced(22, lambda: gs.render(cam, SEED, 0, SPP, slots_per_pixel=1))
        assert ref.shape == (FORMS_H, FORMS_W, 3) and st.shade_variant == 22 and st.n_slots == N_PIXELS and st.samples == N_PIXELS * SPP
        assert st.extend_variant == 0                                   # the two-phase K2: the scene has a mesh
        ref.flags.writeable = False
        REFS[key] = (ref, st)
    return REFS[key]


@pytest.mark.parametrize("sampler", ["independent", "sobol"])
@pytest.mark.parametrize("mode, lights", CASES, ids=[f"{m}-{'lights' if l else 'nolights'}" for m, l in CASES])
def test_every_form_of_k_shade(pt, det, ctx, scenes, mode, lights, sampler):
    qmc = sampler == "sobol"
    ref, rst = reference(scenes, mode, lights, sampler)
    gs, cam, spec = scenes(mode, lights)
    gs.set_sampler(sampler)
    fin = np.isfinite(ref)
    what = f"{mode} lights={lights} {sampler}"

    def ran(st, want, lst):
        """Check 1 for one render, and the record of the form that ran."""
        exists = shade_form_exists(want, lights, lst, qmc, mode)
        assert st.shade_variant == (want if exists else 42), (what, want, lst, st.shade_variant)
        shape = st.shade_variant if exists else {4096: 22, 8192: 32}[window_slots(st)]
        LAUNCHED.add((shape, lights, lst, qmc, mode))

    # the scene keeps the mode's code running
    assert fin.mean() >= 0.99 and ref[fin].max() > 0.0, (what, fin.mean())
    ran(rst, 22, False)
    if mode != "PLAIN":
        plain, _ = reference(scenes, "PLAIN", lights, sampler)
        gs.set_sampler(sampler)
        differs = (~same(ref, plain)).any(axis=2).mean()
        assert differs >= 0.1, (what, differs)

    # 1 (legacy shapes) and 2: static, whole frame
    for v in LEGACY + (32,):
        acc, st = forced(v, lambda: gs.render(cam, SEED, 0, SPP, slots_per_pixel=1))
        ran(st, v, False)
        np.testing.assert_array_equal(acc, ref, err_msg=f"{what}: static whole frame, shape {v}")
        assert (st.segments, st.samples) == (rst.segments, rst.samples), (what, v)
    if mode == "PLAIN" and not qmc:
        assert all((v, lights, False, False, "PLAIN") in LAUNCHED for v in LEGACY)

    # 1 (pixel lists under the legacy shapes) and 3: static pixel lists
    list_counts = {}
    for n in LIST_SIZES:
        sel = pixel_list(n)
        m = mask_of(sel)
        for v in (22, 32) + (LEGACY if n == 100 else ()):
            out, st = forced(v, lambda: gs.render_pixels(cam, SEED, sel, 0, SPP, accum=SENTINEL.copy(), slots_per_pixel=1, overwrite=True))
            ran(st, v, True)
            np.testing.assert_array_equal(out[m], ref[m], err_msg=f"{what}: static list of {n}, shape {v}")
            np.testing.assert_array_equal(out[~m].view(np.uint64), SENTINEL[~m].view(np.uint64), err_msg=f"{what}: unlisted pixels, list of {n}, shape {v}")
            assert st.samples == n * SPP and st.n_slots == n
            assert list_counts.setdefault(n, st.segments) == st.segments, (what, n, v)

    # 4: dynamic mode on the default pool (all work handed out at once) and on a small one
    big = pixel_list(LIST_SIZES[-1])
    mbig = mask_of(big)
    for v in (22, 32):
        for pool in (None, "20000"):
            env = {} if pool is None else {"PT_POOL_SLOTS": pool}
            frames = [("whole frame", False, lambda: gs.render(cam, SEED, 0, SPP), env),
                      ("whole frame in place", False, lambda: gs.render(cam, SEED, 0, SPP), dict(env, PT_POOL_IN_PLACE="1")),
                      ("list", True, lambda: gs.render_pixels(cam, SEED, big, 0, SPP), env)]
            for name, lst, fn, e in frames:
                acc, st = forced(v, fn, **e)
                ran(st, v, lst)
                assert st.slots_per_pixel == 0 and (pool is None or st.n_slots == 20000), (what, v, pool, name)
                keep = fin & mbig[..., None] if lst else fin
                np.testing.assert_allclose(acc[keep], ref[keep], rtol=1e-11, atol=1e-11, err_msg=f"{what}: dynamic {name}, shape {v}, pool {pool}")
                want = (list_counts[len(big)], len(big) * SPP) if lst else (rst.segments, rst.samples)
                assert (st.segments, st.samples) == want, (what, v, pool, name, st.segments, st.samples, want)
                if lst:
                    assert not acc[~mbig].any(), (what, v, pool)

    # 5: adaptive sampling. The threshold is the 0.8 quantile of the first test's error estimate (include/pt_amd.h: samples 0 and 1
    # are the two sets), so about 0.8^9 of the pixels stop there with their whole neighbourhood and most of the others go on.
    (a, _), (b, _) = (forced(22, lambda: gs.render(cam, SEED, i, i + 1, slots_per_pixel=1)) for i in (0, 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(a - b).sum(axis=2) / (1e-4 + np.sqrt((a + b).sum(axis=2) / 2.0))
    thr = float(np.quantile(err[np.isfinite(err)], 0.8))
    assert thr > 0.0, what
    ada = {}
    for v in (22, 32):
        acc, counts, st = forced(v, lambda: gs.render_adaptive(cam, SEED, 2, 8, thr, slots_per_pixel=1))
        ran(st, v, True)
        assert st.samples == int(counts.sum())
        ada[v] = (acc, counts, st.segments)
    assert (ada[22][1] < 8).any() and (ada[22][1] == 8).any(), (what, thr, np.bincount(ada[22][1].reshape(-1)))
    np.testing.assert_array_equal(ada[32][1], ada[22][1], err_msg=f"{what}: adaptive counts")
    np.testing.assert_array_equal(ada[32][0], ada[22][0], err_msg=f"{what}: adaptive sums")
    assert ada[32][2] == ada[22][2]

    print(f"{what}: {rst.segments / rst.samples:.2f} segments per sample, {fin.mean():.4f} finite, differs from PLAIN in "
          f"{differs if mode != 'PLAIN' else 0.0:.3f} of the pixels, adaptive threshold {thr:.4g}: samples per pixel -> pixels "
          f"{dict(zip(*(x.tolist() for x in np.unique(ada[22][1], return_counts=True))))}")

    # 6: the batch K2 in place of the two-phase one
    acc, st = forced(22, lambda: gs.render(cam, SEED, 0, SPP, slots_per_pixel=1), PT_K2="batch")
    assert st.extend_variant == 1 and st.shade_variant == 22
    np.testing.assert_array_equal(acc, ref, err_msg=f"{what}: batch K2")
    assert st.segments == rst.segments

    # 7: the anchor
    if mode == "PLAIN" and not qmc:
        os_ = det.Scene()
        oacc, cnt = os_.render(spec.make_camera(det.Camera, spec.replay(os_)), SEED, 0, SPP)
        os_.close()
        assert cnt["segments"] == rst.segments and cnt["samples"] == rst.samples
        np.testing.assert_array_equal(ref, oacc, err_msg=f"{what}: oracle")
