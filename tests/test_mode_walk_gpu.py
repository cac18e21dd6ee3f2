"""One REUSED scene through every shading mode, pass and rebuild. Every other test renders a scene that is born in its mode and stays
in it; a host keeps one scene and switches features between frames, and a lot of state crosses that boundary: the path pool (never
cleared; its bounce word has five layouts, csrc/pt_types.h), the tiled accumulator with the sky pass's tile map and the short pass's
record behind its planes, the tables kept until destroy (environment tables, dispersion weights), the flags scene_build derives and the
settings written past the build. Here one scene walks the transitions (common.WALK_STATES) and every result is compared with the same
call on a FRESH TWIN: a new scene of the same description that entered that state and nothing else. Both sides are the product, which
is the right oracle for a state leak. Static renders (slots_per_pixel = 1) and probes are order-deterministic: equality is exact.
Dynamic renders are held to the project's bound for dynamic-order f64 sums (test_scene_reuse_gpu.py, test_gpu_parity.py): rtol = atol =
1e-11 on finite pixels, non-finite pixels in the same places, counts exact. tests/test_mode_walk_cpu.py keeps the table complete."""
import numpy as np
import pytest

import common
from common import WALK_STATES

pytestmark = pytest.mark.gpu

SEED = 11
W, H = common.FORMS_W, common.FORMS_H                   # the static frame: three 8192-slot windows
RAGGED = ((100, 76), (200, 148))                        # the dynamic frames, alternating: the tile map behind the planes moves both ways
REGEN = {"PT_EXPERIMENT": "1", "PT_POOL_SLOTS": "4096"}  # a pool far smaller than the frame's samples: K3 regenerates paths in used slots

_rng = np.random.default_rng(20251)
_dirs = _rng.normal(size=(256, 3)) * (0.6, 0.35, 0.0) + (0.0, -0.08, 1.0)
_dirs /= np.linalg.norm(_dirs, axis=1, keepdims=True)
RAYS = np.concatenate([np.broadcast_to((0.0, 1.0, -6.0), _dirs.shape), _dirs, _rng.uniform(0.0, 1.0, (256, 1))], axis=1)
U2 = _rng.uniform(0.0, 1.0, (64, 2))
POINTS = _rng.uniform((-3.0, 0.0, -3.0), (3.0, 3.0, 3.0), (64, 3))
_unit = _rng.normal(size=(64, 3))
_unit /= np.linalg.norm(_unit, axis=1, keepdims=True) * (1.0 + 1e-12)
PHASE_IN = np.concatenate([U2, _unit], axis=1)                                                     # medium_probe 0: (u1, u2, dir)
TRACK_IN = np.concatenate([POINTS, _unit, _rng.uniform(0.5, 6.0, (64, 1))], axis=1)                # medium_probe 3: (o, dir, t)
LENGTHS = _rng.uniform(0.0, 5.0, 64)
LIGHT_IN = np.concatenate([POINTS, _rng.uniform(0.0, 1.0, (64, 1))], axis=1)                       # light_probe 0: (origin, time)
PIX_SAMPLES = np.stack([_rng.integers(0, W * H, 64), _rng.integers(0, 4, 64)], axis=1).astype(np.float64)
LIST_LONG = np.sort(_rng.choice(RAGGED[0][0] * RAGGED[0][1], size=300, replace=False)).astype(np.uint32)   # (valid in both ragged frames)
LIST_SHORT = LIST_LONG[::7][:40].copy()
assert len(LIST_SHORT) == 40


def _make(pt, ctx, lights, extra=()):
    """(scene, camera, handles) of common.mode_walk_scene, built, in the PLAIN state."""
    spec, refs = common.mode_walk_scene(lights, extra)
    gs = pt.Scene(ctx)
    results = spec.replay(gs)
    return gs, spec.make_camera(pt.Camera, results), {k: results[r] for k, r in refs.items()}


def _cam(pt, cam, w, h, **kw):
    c = pt.Camera.from_buffer_copy(cam)
    c.image_width, c.aspect_ratio = w, w / (h + 0.5)      # (height = floor(w / aspect): h + 0.5 keeps a rounding away from h - 1)
    for k, v in kw.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    assert pt.image_height(c) == h
    return c


class Twins:
    """The fresh twins, one per (state, sampler, lights, extra, tag), built once for the module; a twin's answer to a call is computed once.
    `tag`: a twin of its own for calls whose camera decides what scene state they touch (which environment map's tables get built,
    whether the sky pass ever ran), so that it has only ever seen that camera."""

    def __init__(self, pt, ctx):
        self.pt, self.ctx, self.scenes, self.results = pt, ctx, {}, {}

    def scene(self, state, sampler, lights, extra=(), tag=None):
        key = (state, sampler, lights, extra, tag)
        if key not in self.scenes:
            gs, cam, hd = _make(self.pt, self.ctx, lights, extra)
            WALK_STATES[state][0](gs, hd)
            gs.set_sampler(sampler)
            self.scenes[key] = (gs, cam, hd)
        return self.scenes[key]

    def get(self, state, sampler, lights, call, extra=(), tag=None):
        key = (state, sampler, lights, extra, tag, call.key)
        if key not in self.results:
            self.results[key] = call(self.pt, *self.scene(state, sampler, lights, extra, tag))
        return self.results[key]

    def close(self):
        for gs, _, _ in self.scenes.values():
            gs.close()
        self.scenes.clear()


@pytest.fixture(scope="module")
def twins(pt, ctx):
    t = Twins(pt, ctx)
    yield t
    t.close()


# ---- the calls: call(pt, scene, camera, handles) -> (arrays, counts); call.key names it and is the entry point of a failure's message -------
def _call(key, exact=True):
    def wrap(fn):
        fn.key, fn.exact = key, exact
        return fn
    return wrap


def _counts(st):
    return (st.samples, st.segments)


def static(w=W, h=H, begin=0, end=4, **camkw):
    @_call(f"render(static {w}x{h} [{begin},{end}) {sorted(camkw.items())})")
    def call(pt, gs, cam, hd):
        kw = {k: (hd[v] if k == "env_tex" else v) for k, v in camkw.items()}
        acc, st = gs.render(_cam(pt, cam, w, h, **kw), SEED, begin, end, slots_per_pixel=1)
        return (acc,), _counts(st) + (st.shade_variant,)
    return call


def dynamic(w, h, env=None, **camkw):
    @_call(f"render(dynamic {w}x{h} {env} {sorted(camkw.items())})", exact=False)
    def call(pt, gs, cam, hd):
        acc, st = common._with_env(env or {}, lambda: gs.render(_cam(pt, cam, w, h, **camkw), SEED, 0, 4))
        call.stats = st
        return (acc,), _counts(st) + (st.sky_tiles, st.sky_samples, st.short_tiles, st.short_samples, st.hard_samples)
    return call


def pixels(w, h, px):
    @_call(f"render_pixels({w}x{h}, {len(px)} pixels)")
    def call(pt, gs, cam, hd):
        acc, st = gs.render_pixels(_cam(pt, cam, w, h), SEED, px, 0, 4, slots_per_pixel=1)
        return (acc,), _counts(st)
    return call


def aovs(w, h):
    @_call(f"render_aovs({w}x{h})")
    def call(pt, gs, cam, hd):
        return (gs.render_aovs(_cam(pt, cam, w, h), SEED, 0, 2),), ()
    return call


def adaptive(w, h):
    @_call(f"render_adaptive({w}x{h})", exact=False)
    def call(pt, gs, cam, hd):
        acc, counts, st = gs.render_adaptive(_cam(pt, cam, w, h), SEED, 4, 8, 0.05)
        return (acc,), _counts(st) + (counts.tobytes(),)
    return call


@_call("intersect")
def intersect(pt, gs, cam, hd):
    return (gs.intersect(RAYS),), ()


def env_probe(tex="env"):
    @_call(f"env_probe({tex})")
    def call(pt, gs, cam, hd):
        c = _cam(pt, cam, W, H, env_tex=hd[tex])
        return (gs.env_probe(c, 0, U2), gs.env_probe(c, 1, _unit)), ()
    return call


@_call("medium_probe(fog)")
def fog_probe(pt, gs, cam, hd):
    return (gs.medium_probe(hd["fog"], 0, PHASE_IN), gs.medium_probe(hd["fog"], 1, U2[:, 0])), ()


@_call("medium_probe(grid)")
def grid_probe(pt, gs, cam, hd):
    return (gs.medium_probe(hd["grid"], 2, POINTS), gs.medium_probe(hd["grid"], 3, TRACK_IN)), ()


@_call("medium_probe(tinted)")
def tinted_probe(pt, gs, cam, hd):
    return (gs.medium_probe(hd["tinted"], 4, LENGTHS), gs.medium_probe(hd["tinted"], 1, U2[:, 1])), ()


@_call("light_probe")
def light_probe(pt, gs, cam, hd):
    out = gs.light_probe(0, LIGHT_IN)
    return (out, gs.light_probe(1, np.concatenate([POINTS, out[:, :3], LIGHT_IN[:, 3:]], axis=1))), ()


@_call("dispersion_probe")
def dispersion_probe(pt, gs, cam, hd):
    return (gs.dispersion_probe(hd["glass"], 0, PIX_SAMPLES, seed=SEED), gs.dispersion_probe(hd["glass"], 1, np.linspace(400.0, 700.0, 64))), ()


@_call("punctual_probe")
def punctual_probe(pt, gs, cam, hd):
    return (gs.punctual_probe(0, POINTS), gs.punctual_probe(1, np.concatenate([np.arange(64.0)[:, None] % 2, POINTS], axis=1))), ()


# the probe a state owns, on top of intersect
STATE_PROBE = {"ENV": env_probe(), "MED": fog_probe, "HET": grid_probe, "INT": tinted_probe, "INT2": tinted_probe, "LSE": light_probe,
               "DSP": dispersion_probe, "PLT": punctual_probe, "SHF": punctual_probe}


def _differ(a, b):
    """The number of pixels (rows) at which two arrays differ; NaNs in the same place are equal."""
    a, b = np.asarray(a), np.asarray(b)
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    if bad.ndim > 1:      # (H, W, C) images and (n, C) probe rows: a pixel or row differs if any of its last-axis values does
        bad = bad.any(axis=-1)
    return int(np.count_nonzero(bad))


def _same(got, want, prev, cur, call, exact=None):
    """A reused scene's answer against the twin's; the message names the transition, the entry point and the number of differing pixels."""
    exact = call.exact if exact is None else exact
    where = f"{prev} -> {cur}: {call.key}"
    show = lambda t: tuple(x if isinstance(x, int) else "<per-pixel counts>" for x in t)
    assert got[1] == want[1], f"{where}: counts {show(got[1])} != the fresh twin's {show(want[1])}"
    for a, b in zip(got[0], want[0]):
        assert a.shape == b.shape, where
        if exact:
            n = _differ(a, b)
            assert n == 0, f"{where}: {n} of {a.reshape(-1, a.shape[-1]).shape[0] if a.ndim > 1 else a.size} pixels differ from the fresh twin"
        else:
            fin = np.isfinite(b)
            assert np.array_equal(fin, np.isfinite(a)), f"{where}: {int(np.count_nonzero(fin != np.isfinite(a)))} values are non-finite on one side only"
            close = np.isclose(a[fin], b[fin], rtol=1e-11, atol=1e-11)
            assert close.all(), f"{where}: {int(np.count_nonzero(~close))} values differ from the fresh twin beyond rtol = atol = 1e-11 (max abs {np.abs(a[fin] - b[fin]).max():.3e})"


def _switch(gs, hd, prev, cur):
    if prev is not None:
        WALK_STATES[prev][1](gs, hd)
    WALK_STATES[cur][0](gs, hd)


# ---- 1. the precondition: every state is in effect ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lights", [True, False])
def test_fresh_states_all_differ(pt, ctx, twins, lights):
    """The fresh static renders of any two states are different arrays: each state really is in effect, so an equality below means
    something. (RenderStats names no mode; the shape of k_shade it names is part of every comparison.)"""
    states = common.walk_states(lights)
    img = {s: twins.get(s, 0, lights, static())[0][0] for s in states}
    for i, a in enumerate(states):
        assert np.count_nonzero(np.isfinite(img[a]) & (img[a] != 0.0)) > img[a].size // 100, f"the fresh render of {a} is (nearly) black"
        for b in states[i + 1:]:
            assert _differ(img[a], img[b]) > 0, f"the fresh renders of {a} and {b} are equal"
    for s in states:      # ... and the Sobol sampler is in effect in every state (none is in common.WALK_NO_QMC)
        assert _differ(img[s], twins.get(s, 1, lights, static())[0][0]) > 0, f"{s}: the Sobol sampler changes nothing"


# ---- 2. the walk over ordered pairs, static mode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lights", [True, False])
def test_static_walk_over_every_ordered_pair(pt, ctx, twins, lights):
    """An Eulerian circuit of the complete digraph on the states: every (previous, next) pair once, each visit a static render and the
    state's probes, bit-equal to the fresh twin's."""
    states = common.walk_states(lights)
    gs, cam, hd = _make(pt, ctx, lights)
    prev = None
    for cur in common.walk_pair_circuit(states):
        _switch(gs, hd, prev, cur)
        for call in [static(), intersect] + ([STATE_PROBE[cur]] if cur in STATE_PROBE else []):
            _same(call(pt, gs, cam, hd), twins.get(cur, 0, lights, call), prev, cur, call)
        prev = cur
    gs.close()


@pytest.mark.parametrize("lights", [True, False])
def test_static_walk_alternating_samplers(pt, ctx, twins, lights):
    """The shorter second pass: the family walk with three renders per visit, the sampler flipping before every one of them (1, 0, 1 in
    one visit, 0, 1, 0 in the next), so that each sampler's forms follow the other's inside a state and across a switch, both ways."""
    states = common.walk_states(lights)
    assert not common.WALK_NO_QMC      # (a state left out of the sampler axis would be listed there, with its reason)
    gs, cam, hd = _make(pt, ctx, lights)
    prev, sampler, call = None, 0, static()
    for cur in common.walk_family_sequence(states):
        _switch(gs, hd, prev, cur)
        for _ in range(3):
            was = f"{prev} / sampler {sampler}"
            sampler = 1 - sampler
            gs.set_sampler(sampler)
            _same(call(pt, gs, cam, hd), twins.get(cur, sampler, lights, call), was, f"{cur} / sampler {sampler}", call)
            prev = cur
    gs.close()


# ---- 3. the dynamic mode, the passes and the other entry points ------------------------------------------------------------------------------
@pytest.mark.parametrize("lights", [True, False])
def test_dynamic_regeneration_and_entry_points_across_families(pt, ctx, twins, lights):
    """Every state directly after and before a state of another bounce-word layout: a dynamic render whose small pool makes K3 regenerate
    paths in slots the previous mode used, then pixel lists, AOVs and (in PLAIN and MED) an adaptive render, at alternating ragged frames."""
    states = common.walk_states(lights)
    gs, cam, hd = _make(pt, ctx, lights)
    prev = None
    for i, cur in enumerate(common.walk_family_sequence(states)):
        w, h = RAGGED[i % 2]
        _switch(gs, hd, prev, cur)
        calls = [dynamic(w, h, REGEN), pixels(w, h, LIST_LONG), pixels(w, h, LIST_SHORT), aovs(w, h)] + ([adaptive(w, h)] if cur in ("PLAIN", "MED") else [])
        for call in calls:
            _same(call(pt, gs, cam, hd), twins.get(cur, 0, lights, call), prev, cur, call)
        prev = cur
    gs.close()


def test_sky_and_short_pass_switching_on_and_off(pt, ctx, twins):
    """The library's own pool, no lights list, a non-black environment: the sky pass (and the short pass with it) is ON in PLAIN and OFF in
    every other state. PLAIN(on) -> other -> PLAIN(on) at the other frame size, and PLAIN under a black constant environment (pass off, no
    classification at all) between two pass-on renders: that one against a twin of its own, which has never had a pass on, so that a
    stale tile map, hard-list record or list of the previous pass-on render shows."""
    lights = False
    gs, cam, hd = _make(pt, ctx, lights)
    black = dict(env_is_map=0, env_color=(0.0, 0.0, 0.0))
    others = [s for s in common.walk_states(lights) if s != "PLAIN"]
    visits = [("PLAIN", RAGGED[0], {}), ("MED", RAGGED[1], {}), ("PLAIN", RAGGED[1], {}), ("PLAIN", RAGGED[0], black), ("PLAIN", RAGGED[0], {})]
    for i, s in enumerate(others):
        visits += [(s, RAGGED[i % 2], {}), ("PLAIN", RAGGED[(i + 1) % 2], {})]
    prev = None
    for cur, (w, h), camkw in visits:
        _switch(gs, hd, prev, cur)
        call = dynamic(w, h, None, **camkw)
        got = call(pt, gs, cam, hd)
        st = call.stats
        passes = (st.sky_tiles, st.sky_samples, st.short_tiles, st.short_samples, st.hard_samples)
        print(f"{prev} -> {cur} at {w}x{h}{' (black environment)' if camkw else ''}: sky_tiles, sky_samples, short_tiles, short_samples, hard_samples = {passes}")
        if cur == "PLAIN" and not camkw:
            assert all(p > 0 for p in passes), f"{prev} -> {cur}: the sky pass or the short pass is off, or left no hard sample ({passes})"
        else:
            assert passes == (0, 0, 0, 0, 0), f"{prev} -> {cur}: a pass ran ({passes})"
        _same(got, twins.get(cur, 0, lights, call, tag="black" if camkw else None), prev, cur, call)
        prev = cur
    gs.close()


def split_static():
    @_call("render(static [0,2) then [2,4) into one accumulator)")
    def call(pt, gs, cam, hd):
        c = _cam(pt, cam, W, H)
        acc, st0 = gs.render(c, SEED, 0, 2, slots_per_pixel=1)
        acc, st1 = gs.render(c, SEED, 2, 4, accum=acc, slots_per_pixel=1)
        return (acc,), (st0.samples + st1.samples, st0.segments + st1.segments, st1.shade_variant)
    return call


@pytest.mark.parametrize("lights", [True, False])
def test_sample_ranges_across_a_switch(pt, ctx, twins, lights):
    """Samples [0, 2) in state A, another state rendered on the same scene, then [2, 4) in A into the same accumulator. pt_render adds
    the SUM of its range to the frame (include/pt_amd.h), so two ranges associate as (s0 + s1) + (s2 + s3) where one range gives
    ((s0 + s1) + s2) + s3 and the two differ in the last bits of many pixels: against the twin's [0, 4) the counts are exact and the
    sums hold test_gpu_parity.py's bound for sample ranges (rtol = atol = 1e-13). The state-leak check is exact all the same: the twin
    renders the same two ranges with nothing in between, and the reused scene's sum equals that to the bit."""
    seq = common.walk_family_sequence(common.walk_states(lights))
    gs, cam, hd = _make(pt, ctx, lights)
    c = _cam(pt, cam, W, H)
    whole, split = static(), split_static()
    for a, b in zip(seq, seq[1:]):
        WALK_STATES[a][0](gs, hd)
        acc, st0 = gs.render(c, SEED, 0, 2, slots_per_pixel=1)
        _switch(gs, hd, a, b)
        _same(whole(pt, gs, cam, hd), twins.get(b, 0, lights, whole), a, b, whole)
        _switch(gs, hd, b, a)
        acc, st1 = gs.render(c, SEED, 2, 4, accum=acc, slots_per_pixel=1)
        got = ((acc,), (st0.samples + st1.samples, st0.segments + st1.segments, st1.shade_variant))
        _same(got, twins.get(a, 0, lights, split), f"{a} [0,2) -> {b}", f"{a} [2,4)", split)
        ref = twins.get(a, 0, lights, whole)
        assert got[1] == ref[1], f"{a} [0,2) -> {b} -> {a} [2,4): counts {got[1]} != the twin's [0,4) {ref[1]}"
        fin = np.isfinite(ref[0][0])
        assert np.array_equal(fin, np.isfinite(acc))
        np.testing.assert_allclose(acc[fin], ref[0][0][fin], rtol=1e-13, atol=1e-13, err_msg=f"{a} [0,2) -> {b} -> {a} [2,4) against the twin's [0,4)")
        WALK_STATES[a][1](gs, hd)
    gs.close()


# ---- 4. tables kept until destroy ----------------------------------------------------------------------------------------------------------------
def test_environment_tables_follow_the_map(pt, ctx, twins):
    """The environment tables are keyed by the texture handle: 8x4 map, 16x8 map, all-zero map, 8x4 again on one scene with sampling on,
    then once more after a rebuild that moved every earlier texture's atlas offset. Every step is compared with a twin that has only ever
    seen that step's map (its tables cannot be another map's). The zero map has Z = 0: it renders exactly like sampling off, and has
    no probe."""
    lights = True
    gs, cam, hd = _make(pt, ctx, lights)
    gs.set_env_sampling(0.5)
    prev = None
    for step, tex in enumerate(("env", "env2", "env0", "env", "rebuild", "env")):
        if tex == "rebuild":
            gs.tex_image_rgbf32(np.full((5, 3, 3), 0.25, dtype=np.float32))
            with pytest.raises(pt.PtError, match="world not built"):
                gs.env_probe(_cam(pt, cam, W, H), 0, U2)
            gs.world_build()
            prev = "ENV(rebuilt)"
            continue
        call = static(env_tex=tex)
        _same(call(pt, gs, cam, hd), twins.get("ENV", 0, lights, call, tag=tex), prev, f"ENV({tex})", call)
        if tex == "env0":
            _same(call(pt, gs, cam, hd), twins.get("PLAIN", 0, lights, call, tag=tex), prev, "ENV(env0) against sampling off", call)
            with pytest.raises(pt.PtError, match="Z = 0"):
                gs.env_probe(_cam(pt, cam, W, H, env_tex=hd[tex]), 0, U2)
        else:
            probe = env_probe(tex)
            _same(probe(pt, gs, cam, hd), twins.get("ENV", 0, lights, probe, tag=tex), prev, f"ENV({tex})", probe)
        prev = f"ENV({tex})"
    assert _differ(twins.get("ENV", 0, lights, static(env_tex="env"), tag="env")[0][0], twins.get("ENV", 0, lights, static(env_tex="env2"), tag="env2")[0][0]) > 0
    gs.close()


def _extra_ball(add, hd):
    add("world_add_object", add("sphere", 0.3, (1.0, 2.4, -0.5), (1.0, 2.4, -0.5), hd["metal"]))


def test_dispersion_table_survives_a_rebuild(pt, ctx, twins):
    """DSP -> leave -> another object and a rebuild -> DSP again, the dispersion probe each time."""
    lights = True
    gs, cam, hd = _make(pt, ctx, lights)
    calls = (static(), dispersion_probe, intersect)
    _switch(gs, hd, None, "DSP")
    for call in calls:
        _same(call(pt, gs, cam, hd), twins.get("DSP", 0, lights, call), None, "DSP", call)
    _switch(gs, hd, "DSP", "PLAIN")
    _extra_ball(gs.call, hd)
    gs.world_build()
    _same(calls[0](pt, gs, cam, hd), twins.get("PLAIN", 0, lights, calls[0], extra=(_extra_ball,)), "DSP", "PLAIN(one more object)", calls[0])
    _switch(gs, hd, "PLAIN", "DSP")
    for call in calls:
        _same(call(pt, gs, cam, hd), twins.get("DSP", 0, lights, call, extra=(_extra_ball,)), "PLAIN(one more object)", "DSP", call)
    gs.close()


def _extra_plt_03(add, hd):
    """PLT with the fraction 0.3, all ahead of the scene's only build."""
    add("set_punctual_fraction", 0.3)
    add("light_point", *common.WALK_POINT)
    add("light_spot", *common.WALK_SPOT)


def test_punctual_fraction_survives_a_rebuild(pt, ctx, twins):
    """set_punctual_fraction writes into the device view past the build: set 0.3, rebuild, render PLT; the twin set 0.3, and made its
    lights, before its only build. The fraction is in effect: the default's render differs."""
    lights = True
    gs, cam, hd = _make(pt, ctx, lights)
    gs.set_punctual_fraction(0.3)
    gs.world_build()
    _switch(gs, hd, None, "PLT")
    assert gs.punctual_fraction() == 0.3
    for call in (static(), punctual_probe):
        _same(call(pt, gs, cam, hd), twins.get("PLAIN", 0, lights, call, extra=(_extra_plt_03,)), "PLAIN(f = 0.3, rebuilt)", "PLT", call)
    assert _differ(twins.get("PLAIN", 0, lights, static(), extra=(_extra_plt_03,))[0][0], twins.get("PLT", 0, lights, static())[0][0]) > 0
    gs.set_punctual_fraction(0.5)      # ... and takes effect at once, without a rebuild
    _same(static()(pt, gs, cam, hd), twins.get("PLT", 0, lights, static()), "PLT(f = 0.3)", "PLT(f = 0.5)", static())
    gs.close()


# ---- 5. rebuilds, and what "takes effect at the next build" means ---------------------------------------------------------------------------------
def _extra_growth(add, hd):
    """A sphere, an instanced icosphere(2) mesh (320 triangles) and one more light."""
    add("world_add_object", add("sphere", 0.4, (-2.6, 1.9, 1.2), (-2.6, 1.9, 1.2), hd["glass"]))
    P, I = common.icosphere(2)
    add("world_add_object", add("instance", add("mesh", 0.5, P, I, None, None, hd["metal"]), (0.2, 1.0, 0.1), 0.5, (2.6, 1.8, 0.2)))
    add("world_add_light", add("quad", (1.5, 3.5, -1.0), (0.8, 0.0, 0.0), (0.0, 0.0, 0.8), add("mat_light", add("tex_solid_rgb", 6.0, 5.0, 9.0))))


@pytest.mark.parametrize("lights", [True, False])
def test_rebuilding_a_scene_that_has_rendered(pt, ctx, twins, lights):
    gs, cam, hd = _make(pt, ctx, lights)
    calls = (static(), intersect)
    for call in calls:
        _same(call(pt, gs, cam, hd), twins.get("PLAIN", 0, lights, call), None, "PLAIN", call)
    _extra_growth(gs.call, hd)
    for refused in (lambda: gs.render(_cam(pt, cam, W, H), SEED, 0, 4, slots_per_pixel=1), lambda: gs.intersect(RAYS), lambda: gs.env_probe(_cam(pt, cam, W, H), 0, U2)):
        with pytest.raises(pt.PtError, match="world not built"):      # refused, and the scene stays usable
            refused()
    gs.world_build()
    assert gs.device_bvh_info()[0] == 0
    for call in calls:
        _same(call(pt, gs, cam, hd), twins.get("PLAIN", 0, lights, call, extra=(_extra_growth,)), "PLAIN", "PLAIN(grown, rebuilt)", call)
    assert _differ(twins.get("PLAIN", 0, lights, calls[0], extra=(_extra_growth,))[0][0], twins.get("PLAIN", 0, lights, calls[0])[0][0]) > 0
    gs.set_device_bvh_threshold(100)      # clears `built`; the closest hit does not depend on the tree
    with pytest.raises(pt.PtError, match="world not built"):
        gs.render(_cam(pt, cam, W, H), SEED, 0, 4, slots_per_pixel=1)
    gs.world_build()
    assert gs.device_bvh_info()[0] == 1, "the one mesh of at least 100 triangles: icosphere(2)'s 320 (icosphere(1) has 80, the light mesh 20)"
    for call in calls:
        _same(call(pt, gs, cam, hd), twins.get("PLAIN", 0, lights, call, extra=(_extra_growth,)), "PLAIN(grown)", "PLAIN(device BVH)", call)
    gs.close()


def test_punctual_list_takes_effect_at_the_next_build(pt, ctx, twins):
    """include/pt_amd.h: "The list takes effect at the next pt_world_build", "In effect: n > 0 at the last build". Pinned both ways:
    clearing the list and adding to it change nothing until the rebuild."""
    lights = True
    gs, cam, hd = _make(pt, ctx, lights)
    call = static()
    _switch(gs, hd, None, "PLT")
    before = call(pt, gs, cam, hd)
    _same(before, twins.get("PLT", 0, lights, call), None, "PLT", call)
    gs.clear_punctual_lights()
    assert gs.punctual_count() == 0
    _same(call(pt, gs, cam, hd), before, "PLT", "PLT(list cleared, not rebuilt)", call)
    _same(punctual_probe(pt, gs, cam, hd), twins.get("PLT", 0, lights, punctual_probe), "PLT", "PLT(list cleared, not rebuilt)", punctual_probe)
    gs.world_build()
    _same(call(pt, gs, cam, hd), twins.get("PLAIN", 0, lights, call), "PLT(list cleared)", "PLAIN(rebuilt)", call)
    assert gs.light_point(*common.WALK_POINT) == 0 and gs.punctual_count() == 1
    _same(call(pt, gs, cam, hd), twins.get("PLAIN", 0, lights, call), "PLAIN", "PLAIN(a light added, not rebuilt)", call)
    with pytest.raises(pt.PtError, match="built without punctual lights"):
        gs.punctual_probe(0, POINTS)
    gs.light_spot(*common.WALK_SPOT)
    gs.world_build()
    _same(call(pt, gs, cam, hd), twins.get("PLT", 0, lights, call), "PLAIN(lights added)", "PLT(rebuilt)", call)
    gs.close()


@pytest.mark.parametrize("setter", ["mat_glass_set_interior", "mat_glass_set_dispersion", "set_device_bvh_threshold", "push"])
def test_calls_after_a_setter_that_cleared_built_are_refused(pt, ctx, twins, setter):
    lights = True
    gs, cam, hd = _make(pt, ctx, lights)
    call = static()
    _same(call(pt, gs, cam, hd), twins.get("PLAIN", 0, lights, call), None, "PLAIN", call)
    state = {"mat_glass_set_interior": "INT2", "mat_glass_set_dispersion": "DSP"}.get(setter, "PLAIN")
    if setter == "mat_glass_set_interior":
        gs.mat_glass_set_interior(hd["glass"], hd["tinted"])
    elif setter == "mat_glass_set_dispersion":
        gs.mat_glass_set_dispersion(hd["glass"], 30.0)
    elif setter == "set_device_bvh_threshold":
        gs.set_device_bvh_threshold(1 << 19)
    else:
        gs.tex_solid_rgb(0.1, 0.2, 0.3)
    c = _cam(pt, cam, W, H)
    refused = [lambda: gs.render(c, SEED, 0, 4, slots_per_pixel=1), lambda: gs.render_pixels(c, SEED, LIST_SHORT, 0, 4, slots_per_pixel=1), lambda: gs.render_aovs(c, SEED, 0, 2),
               lambda: gs.render_adaptive(c, SEED, 4, 8, 0.05), lambda: gs.intersect(RAYS), lambda: gs.env_probe(c, 0, U2), lambda: gs.light_probe(0, LIGHT_IN),
               lambda: gs.punctual_probe(0, POINTS)]
    for f in refused:
        with pytest.raises(pt.PtError, match="world not built"):
            f()
    gs.world_build()
    for call in (static(), intersect):
        _same(call(pt, gs, cam, hd), twins.get(state, 0, lights, call), f"PLAIN({setter}, refused calls)", state, call)
    gs.close()


def test_two_live_scenes_on_one_context(pt, ctx, twins):
    """A (MED) and B (PLT) alternate on one context at different frame sizes, static and dynamic: each render equals its twin's."""
    lights = True
    a, b = _make(pt, ctx, lights), _make(pt, ctx, lights)
    WALK_STATES["MED"][0](a[0], a[2])
    WALK_STATES["PLT"][0](b[0], b[2])
    prev = None
    for rnd in range(2):
        for name, (gs, cam, hd), (w, h) in (("MED", a, RAGGED[rnd]), ("PLT", b, RAGGED[1 - rnd])):
            for call in (static(w, h), dynamic(w, h, REGEN)):
                _same(call(pt, gs, cam, hd), twins.get(name, 0, lights, call), f"{prev} (the other scene)", name, call)
            prev = name
    a[0].close()
    b[0].close()
