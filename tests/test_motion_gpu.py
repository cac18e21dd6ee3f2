"""Motion blur of instances on the GPU (pt_instance_moving, pt_scene_set_shutter; the rule is in include/pt_amd.h).
The anchor is the rule's identity: a moving instance at time t IS the static pt_instance of the two lerped values, bit for bit. One
scene is recorded once and replayed as the moving scene, as its static twin posed at a time t (pt_instance with numpy-lerped
arguments, moving spheres pinned at their centre of that time), with every instance declared moving with equal keys, and plain; the
twins replay into the oracle too. A truly moving scene frozen at t != 0 cannot pass on the kernels without motion: InstD holds the pose
at time 0."""
import numpy as np
import pytest

import motion_rule as MR
from common import SceneSpec, _with_env, default_camera, icosphere

pytestmark = pytest.mark.gpu

SEED, SPP, W, H = 11, 4, 96, 64          # 6144 slots in static mode: one full 4096-slot window and one half-live
TIMES = (0.37, 1.0)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return tuple(v / np.linalg.norm(v))


class Recorder:
    """mode "moving": instance_moving and moving spheres as written; ("twin", t): the static scene posed at time t; "equal": every instance
    declared moving with its first key twice, spheres still; "plain": the first keys, static. `placements`: per world entry (lights first,
    then objects) the object-space points of its primitives as a function of time and its chain of keys, outermost first."""

    def __init__(self, mode):
        self.mode, self.t = (mode[0], mode[1]) if isinstance(mode, tuple) else (mode, None)
        self.s = SceneSpec()
        self.geom = {}                     # object ref -> (points(t), chain)
        self.lights, self.objects = [], []

    def add(self, *a):
        return self.s.add(*a)

    def _leaf(self, ref, points):
        self.geom[int(ref)] = (points, [])
        return ref

    def sphere(self, r, p1, p2, mat):
        p1, p2 = np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)
        if self.mode == "twin":
            p1 = p2 = p1 + (p2 - p1) * np.float64(self.t)
        elif self.mode in ("equal", "plain"):
            p2 = p1
        a, b = p1.copy(), p2.copy()
        offs = np.concatenate([np.eye(3), -np.eye(3)]) * r
        return self._leaf(self.add("sphere", r, tuple(p1), tuple(p2), mat), lambda t: (a + (b - a) * t) + offs)

    def quad(self, q, u, v, mat):
        q, u, v = (np.asarray(x, dtype=np.float64) for x in (q, u, v))
        pts = np.array([q, q + u, q + v, q + u + v])
        return self._leaf(self.add("quad", tuple(q), tuple(u), tuple(v), mat), lambda t: pts)

    def cuboid(self, a, b, mat):
        pts = MR.corners(np.concatenate([np.minimum(a, b), np.maximum(a, b)]))
        return self._leaf(self.add("cuboid", tuple(a), tuple(b), mat), lambda t: pts)

    def mesh(self, scale, P, I, mat):
        pts = np.asarray(P, dtype=np.float32).astype(np.float64) * scale
        return self._leaf(self.add("mesh", scale, P, I, None, None, mat), lambda t: pts)

    def inst(self, obj, axis, a0, a1, tr0, tr1):
        """a moving instance of the moving scene"""
        if self.mode == "moving":
            ref = self.add("instance_moving", obj, axis, a0, a1, tr0, tr1)
        elif self.mode == "twin":
            angle, tr = MR.lerp_keys(a0, a1, tr0, tr1, self.t)
            ref = self.add("instance", obj, axis, float(angle), tuple(float(x) for x in tr))
        elif self.mode == "equal":
            ref = self.add("instance_moving", obj, axis, a0, a0, tr0, tr0)
        else:
            ref = self.add("instance", obj, axis, a0, tr0)
        pts, chain = self.geom[int(obj)]
        self.geom[int(ref)] = (pts, [(axis, a0, a1, tr0, tr1)] + chain)
        return ref

    def still(self, obj, axis, angle, tr):
        """a static instance of the moving scene"""
        ref = self.add("instance_moving", obj, axis, angle, angle, tr, tr) if self.mode == "equal" else self.add("instance", obj, axis, angle, tr)
        pts, chain = self.geom[int(obj)]
        self.geom[int(ref)] = (pts, [(axis, angle, angle, tr, tr)] + chain)
        return ref

    def place(self, obj, light=False):
        (self.lights if light else self.objects).append(self.geom[int(obj)])
        self.add("world_add_light" if light else "world_add_object", obj)

    @property
    def placements(self):
        return self.lights + self.objects


def record(mode, tree=False, cuboids=True, lights=True):
    """The test scene: a still and a moving sphere, a moving-instanced quad and cuboid, icosphere(1) as ONE mesh placed still, translating
    and spinning + translating, three nested chains (moving -> static -> mesh, static -> moving -> cuboid, moving -> moving -> sphere) and a
    moving-instanced quad light in the lights list: 12 entries, a flat top level; `tree`: 20 more still spheres, so the top level is a tree;
    cuboids = False: quads in their place (the batch K2 without pair passes)."""
    r = Recorder(mode)
    rgb = lambda a, b, c: r.add("tex_solid_rgb", a, b, c)
    floor = r.add("mat_diffuse", r.add("tex_checker", 0.7, rgb(0.2, 0.3, 0.1), rgb(0.9, 0.9, 0.9)), -1)
    metal = r.add("mat_metal", rgb(0.85, 0.75, 0.5), r.add("tex_solid_f", 0.15))
    red, blue, green = (r.add("mat_diffuse", rgb(*c), -1) for c in ((0.8, 0.2, 0.15), (0.2, 0.3, 0.8), (0.2, 0.7, 0.3)))
    X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    box = (lambda a, b, m: r.cuboid(a, b, m)) if cuboids else (lambda a, b, m: r.quad(a, (b[0] - a[0], 0.0, 0.0), (0.0, b[1] - a[1], 0.0), m))
    r.place(r.quad((-20.0, 0.0, -20.0), (0.0, 0.0, 40.0), (40.0, 0.0, 0.0), floor))
    r.place(r.sphere(0.5, (-2.4, 0.5, 0.6), (-2.4, 0.5, 0.6), metal))
    r.place(r.sphere(0.35, (2.2, 0.4, -0.8), (2.6, 0.9, -0.8), red))
    r.place(r.inst(r.quad((-0.5, 0.0, -0.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), green), Y, 0.2, 0.9, (-1.2, 0.3, 1.8), (-0.8, 0.5, 1.6)))
    r.place(r.inst(box((0.0, 0.0, 0.0), (0.6, 0.8, 0.6), red), Y, 0.3, 0.8, (0.9, 0.0, 1.2), (1.3, 0.1, 1.0)))
    P, I = icosphere(1)
    mesh = r.mesh(0.45, P, I, blue)
    r.place(r.still(mesh, Y, 0.3, (-0.6, 0.5, -0.2)))
    r.place(r.inst(mesh, Y, 0.4, 0.4, (0.6, 0.45, -0.6), (1.0, 0.6, -0.4)))                                # translates only
    r.place(r.inst(mesh, unit((0.3, 0.9, 0.2)), -0.5, 0.7, (-0.3, 1.5, 0.4), (0.1, 1.7, 0.2)))
    r.place(r.inst(r.still(mesh, X, 0.9, (0.0, 0.2, 0.0)), Z, -0.3, 0.2, (2.0, 1.4, 1.0), (1.7, 1.6, 1.2)))
    r.place(r.still(r.inst(box((-0.3, 0.0, -0.3), (0.3, 0.7, 0.3), green), Y, 0.0, 0.6, (0.0, 0.0, 0.0), (0.2, 0.0, 0.1)), Y, 0.3, (-2.2, 0.0, 2.4)))
    ball = r.sphere(0.3, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), metal)
    r.place(r.inst(r.inst(ball, X, 0.0, 1.0, (0.3, 0.0, 0.0), (0.5, 0.1, 0.0)), Y, 0.2, -0.4, (-1.5, 2.0, 0.5), (-1.2, 2.2, 0.3)))
    if tree:
        for k in range(20):
            c = (-3.0 + 0.3 * k, 0.12, -1.8 + 0.05 * (k % 4))
            r.place(r.sphere(0.12, c, c, red))
    if lights:
        lm = r.add("mat_light", rgb(9.0, 8.0, 7.0))
        r.place(r.inst(r.quad((-0.6, 0.0, -0.6), (1.2, 0.0, 0.0), (0.0, 0.0, 1.2), lm), X, 0.1, 0.3, (0.0, 4.0, 0.0), (0.4, 4.1, 0.2)), light=True)
    r.add("world_build")
    r.s.camera = default_camera(width=W, aspect=W / H, spp=SPP, look_from=(0.0, 2.0, -6.5), look_at=(0.0, 0.9, 0.0), vfov=45.0, env_color=(0.05, 0.06, 0.09))
    return r


@pytest.fixture(scope="module")
def scenes(pt, ctx):
    """GPU scenes by (mode, tree, cuboids), built once: (scene, camera, recorder)."""
    cache = {}

    def get(mode, tree=False, cuboids=True):
        key = (mode, tree, cuboids)
        if key not in cache:
            rec = record(mode, tree, cuboids)
            gs = pt.Scene(ctx)
            res = rec.s.replay(gs)
            cache[key] = (gs, rec.s.make_camera(pt.Camera, res), rec)
        return cache[key]

    yield get
    for gs, _, _ in cache.values():
        gs.close()


@pytest.fixture(scope="module")
def oracle_twin(orc):
    """The deterministic-math oracle's render of a twin, computed once per (t, tree, cuboids) and left unchanged."""
    cache = {}

    def get(t, tree=False, cuboids=True):
        key = (t, tree, cuboids)
        if key not in cache:
            orc.set_math_mode(True)
            try:
                rec = record(("twin", t), tree, cuboids)
                os_ = orc.Scene()
                res = rec.s.replay(os_)
                ref, cnt = os_.render(rec.s.make_camera(orc.Camera, res), SEED, 0, SPP)
                os_.close()
            finally:
                orc.set_math_mode(False)
            ref.setflags(write=False)
            cache[key] = (ref, cnt["segments"])
        return cache[key]

    return get


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and (bits(a) == bits(b)).all()


def frozen(gs, t):
    gs.set_shutter(t, t)
    assert gs.motion()
    return gs


# ---- 1: the probes --------------------------------------------------------------------------------------------------------------------
def probe_rays(n, t, seed):
    rng = np.random.default_rng(seed)
    o = np.array([0.0, 2.0, -6.5]) + rng.uniform(-1.5, 1.5, size=(n, 3))
    target = np.stack([rng.uniform(-3.0, 3.0, size=n), rng.uniform(0.0, 2.5, size=n), rng.uniform(-2.0, 3.0, size=n)], axis=1)
    o[n // 2:] = target[n // 2:] + rng.normal(size=(n - n // 2, 3)) * 2.0     # and rays that start among the objects
    return np.concatenate([o, target - o, np.full((n, 1), t)], axis=1)


@pytest.mark.parametrize("tree", [False, True], ids=["flat", "tree"])
@pytest.mark.parametrize("t", [0.0, 0.37, 1.0])
def test_probes_equal_the_static_twin(scenes, t, tree):
    gs, _, _ = scenes("moving", tree)
    tw, _, _ = scenes(("twin", t), tree)
    rays = probe_rays(4096, t, 3)
    a, b = gs.intersect(rays), tw.intersect(rays)
    assert 0.3 < a[:, 0].mean() and len(np.unique(a[a[:, 0] == 1.0, 2])) > 40, "the rays must reach every kind of placement"
    assert same_bits(a, b), f"{(bits(a) != bits(b)).any(axis=1).sum()} of 4096 rays differ"
    rng = np.random.default_rng(4)
    origins = np.stack([rng.uniform(-3.0, 3.0, size=4096), rng.uniform(0.0, 3.0, size=4096), rng.uniform(-2.0, 3.0, size=4096)], axis=1)
    q = np.concatenate([origins, np.full((4096, 1), t)], axis=1)
    sa, sb = gs.light_probe(0, q), tw.light_probe(0, q)
    assert same_bits(sa, sb)
    p = np.concatenate([origins, sa[:, :3], np.full((4096, 1), t)], axis=1)
    pa, pb = gs.light_probe(1, p), tw.light_probe(1, p)
    assert (pa > 0.0).mean() > 0.9 and same_bits(pa, pb)


# ---- 2: frozen renders ------------------------------------------------------------------------------------------------------------------
EXP = {"PT_EXPERIMENT": "1"}
CONFIGS = {   # name -> (tree, cuboids, environment); every one is compared with the twin AND with the oracle's render of the twin
    "default": (False, True, {}),
    "batch": (False, True, dict(EXP, PT_K2="batch")),
    "tree": (True, True, {}),
    "tree-batch": (True, True, dict(EXP, PT_K2="batch")),
    "no-cuboids-batch": (False, False, dict(EXP, PT_K2="batch")),
    "ext2-204": (False, True, dict(EXP, PT_EXT2="204")),
    "ext2-243": (False, True, dict(EXP, PT_EXT2="243")),
    "ext2-283": (False, True, dict(EXP, PT_EXT2="283")),
    "ext2-323": (False, True, dict(EXP, PT_EXT2="323")),
    "shape-32": (False, True, dict(EXP, PT_SHADE_VARIANT="32")),
}


@pytest.mark.parametrize("t", TIMES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_frozen_render_equals_the_twin_and_the_oracle(scenes, oracle_twin, config, t):
    tree, cuboids, env = CONFIGS[config]
    gs, cam, _ = scenes("moving", tree, cuboids)
    tw, tcam, _ = scenes(("twin", t), tree, cuboids)
    frozen(gs, t)
    assert not tw.motion()
    acc, st = _with_env(env, lambda: gs.render(cam, SEED, 0, SPP, slots_per_pixel=1))
    ref, rst = _with_env(env, lambda: tw.render(tcam, SEED, 0, SPP, slots_per_pixel=1))
    assert st.samples == rst.samples == W * H * SPP and st.segments == rst.segments
    assert st.extend_variant == rst.extend_variant == (1 if "batch" in config else 0)
    assert same_bits(acc, ref), f"{(bits(acc) != bits(ref)).any(axis=2).sum()} pixels differ from the twin's"
    oref, osegs = oracle_twin(t, tree, cuboids)
    assert st.segments == osegs and same_bits(acc, oref), f"{(bits(acc) != bits(oref)).any(axis=2).sum()} pixels differ from the oracle's"


@pytest.mark.parametrize("t", TIMES)
def test_frozen_render_sobol_list_adaptive_aovs(pt, scenes, oracle_twin, t):
    gs, cam, _ = scenes("moving")
    tw, tcam, _ = scenes(("twin", t))
    frozen(gs, t)
    # the Sobol sampler, against the twin only (the oracle has none)
    for s in (gs, tw):
        s.set_sampler("sobol")
    try:
        acc, st = gs.render(cam, SEED, 0, SPP, slots_per_pixel=1)
        ref, rst = tw.render(tcam, SEED, 0, SPP, slots_per_pixel=1)
        aov, raov = gs.render_aovs(cam, SEED, 0, SPP), tw.render_aovs(tcam, SEED, 0, SPP)
    finally:
        for s in (gs, tw):
            s.set_sampler("independent")
    assert st.segments == rst.segments and same_bits(acc, ref) and same_bits(aov, raov)
    # a 3000-pixel list
    pixels = np.sort(np.random.default_rng(5).choice(W * H, size=3000, replace=False))
    acc, st = gs.render_pixels(cam, SEED, pixels, 0, SPP, slots_per_pixel=1)
    ref, rst = tw.render_pixels(tcam, SEED, pixels, 0, SPP, slots_per_pixel=1)
    assert st.samples == 3000 * SPP and st.segments == rst.segments and same_bits(acc, ref)
    oref = oracle_twin(t)[0].reshape(-1, 3)                                 # the static mode is per pixel: the oracle's image at the listed pixels
    listed = np.zeros(W * H, dtype=bool)
    listed[pixels] = True
    assert same_bits(acc.reshape(-1, 3)[listed], oref[listed]) and not acc.reshape(-1, 3)[~listed].any()
    # adaptive sampling: the same pixels stop at the same counts
    acc, counts, st = gs.render_adaptive(cam, SEED, 4, 12, 0.05, slots_per_pixel=1)
    ref, rcounts, rst = tw.render_adaptive(tcam, SEED, 4, 12, 0.05, slots_per_pixel=1)
    assert (counts == rcounts).all() and 4 <= counts.min() < counts.max() and st.segments == rst.segments and same_bits(acc, ref)
    # the first-hit feature buffers
    aov, raov = gs.render_aovs(cam, SEED, 0, SPP), tw.render_aovs(tcam, SEED, 0, SPP)
    assert aov[..., 7].sum() > 0.5 * W * H * SPP and same_bits(aov, raov)


@pytest.mark.parametrize("t", TIMES)
@pytest.mark.parametrize("pool", [None, "5000"])
def test_frozen_render_dynamic_mode(scenes, t, pool):
    """The dynamic mode adds the same contributions in another order: rtol = atol = 1e-11, the project's bound for reordered sums, and
    equal counts."""
    gs, cam, _ = scenes("moving")
    tw, tcam, _ = scenes(("twin", t))
    frozen(gs, t)
    ref, rst = tw.render(tcam, SEED, 0, SPP, slots_per_pixel=1)
    env = dict(EXP, PT_POOL_SLOTS=pool) if pool else {}
    acc, st = _with_env(env, lambda: gs.render(cam, SEED, 0, SPP))
    assert st.slots_per_pixel == 0 and st.samples == rst.samples and st.segments == rst.segments
    if pool:
        assert st.n_slots == 5000
    np.testing.assert_allclose(acc, ref, rtol=1e-11, atol=1e-11)


def spheres_only(mode, t=None):
    """Motion through the shutter alone: moving spheres, a static instance, no instance made by pt_instance_moving (SceneD::inst_motion is null)."""
    r = Recorder((mode, t) if mode == "twin" else mode)
    rgb = lambda a, b, c: r.add("tex_solid_rgb", a, b, c)
    floor = r.add("mat_diffuse", r.add("tex_checker", 0.7, rgb(0.2, 0.3, 0.1), rgb(0.9, 0.9, 0.9)), -1)
    red, metal = r.add("mat_diffuse", rgb(0.8, 0.2, 0.15), -1), r.add("mat_metal", rgb(0.85, 0.75, 0.5), r.add("tex_solid_f", 0.15))
    r.place(r.quad((-20.0, 0.0, -20.0), (0.0, 0.0, 40.0), (40.0, 0.0, 0.0), floor))
    r.place(r.sphere(0.5, (-1.5, 0.5, 0.5), (-0.7, 1.1, 0.3), red))
    r.place(r.sphere(0.4, (1.2, 0.4, -0.5), (1.9, 0.4, 0.4), metal))
    P, I = icosphere(1)
    r.place(r.still(r.mesh(0.45, P, I, red), (0.0, 1.0, 0.0), 0.3, (0.2, 0.5, 1.5)))
    r.place(r.quad((-0.6, 4.0, -0.6), (1.2, 0.0, 0.0), (0.0, 0.0, 1.2), r.add("mat_light", rgb(9.0, 8.0, 7.0))), light=True)
    r.add("world_build")
    r.s.camera = default_camera(width=W, aspect=W / H, spp=SPP, look_from=(0.0, 2.0, -6.5), look_at=(0.0, 0.9, 0.0), vfov=45.0, env_color=(0.05, 0.06, 0.09))
    return r


@pytest.mark.parametrize("t", TIMES)
def test_the_shutter_scales_moving_spheres(pt, ctx, orc, t):
    """No moving instance: motion is in effect only once the shutter is not (0, 1), the MOT kernels run with a null motion table, and the
    frozen render is the pinned twin's and the oracle's, static and dynamic mode."""
    built = []
    try:
        for rec in (spheres_only("moving"), spheres_only("twin", t)):
            gs = pt.Scene(ctx)
            built.append((gs, rec.s.make_camera(pt.Camera, rec.s.replay(gs))))
        (gs, cam), (tw, tcam) = built
        assert not gs.motion() and not tw.motion()                          # the default shutter: nothing new runs
        gs.set_shutter(t, t)
        assert gs.motion()
        tw.set_shutter(t, t)
        assert not tw.motion()                                               # nothing moves there
        acc, st = gs.render(cam, SEED, 0, SPP, slots_per_pixel=1)
        ref, rst = tw.render(tcam, SEED, 0, SPP, slots_per_pixel=1)
        assert st.segments == rst.segments and same_bits(acc, ref)
        orc.set_math_mode(True)
        try:
            rec = spheres_only("twin", t)
            os_ = orc.Scene()
            oref, cnt = os_.render(rec.s.make_camera(orc.Camera, rec.s.replay(os_)), SEED, 0, SPP)
            os_.close()
        finally:
            orc.set_math_mode(False)
        assert st.segments == cnt["segments"] and same_bits(acc, oref)
        dyn, dst = gs.render(cam, SEED, 0, SPP)
        assert dst.segments == st.segments
        np.testing.assert_allclose(dyn, ref, rtol=1e-11, atol=1e-11)
        # a shutter that is open for a part of the interval keeps every time inside it
        gs.set_shutter(0.25, 0.5)
        rays = gs.camera_probe(cam, SEED, np.stack([np.arange(2048) % (W * H), np.arange(2048) // 64], axis=1))
        assert 0.25 <= rays[:, 6].min() and rays[:, 6].max() <= 0.5 and rays[:, 6].max() - rays[:, 6].min() > 0.2
    finally:
        for gs, _ in built:
            gs.close()


# ---- 3: equal keys ------------------------------------------------------------------------------------------------------------------------
def test_equal_keys_render_the_plain_scene(scenes):
    gs, cam, _ = scenes("equal")
    pl, pcam, _ = scenes("plain")
    gs.set_shutter(0.0, 1.0)
    assert gs.motion() and not pl.motion() and gs.shutter() == (0.0, 1.0)
    acc, st = gs.render(cam, SEED, 0, SPP, slots_per_pixel=1)
    ref, rst = pl.render(pcam, SEED, 0, SPP, slots_per_pixel=1)
    assert st.segments == rst.segments and same_bits(acc, ref)


# ---- 4: blur is there and is exact -----------------------------------------------------------------------------------------------------
BW, BH, BSPP, BSEED = 64, 48, 64, 8
B_QUAD = ((-0.6, -1.8, 0.0), (1.2, 0.0, 0.0), (0.0, 3.6, 0.0))
B_KEYS = ((0.0, 0.0, 1.0), 0.0, float(np.radians(40.0)), (-1.65, 0.0, 0.0), (1.65, 0.0, 0.0))   # across a third of the 9.9-wide frame, a 40 degree spin


def blur_scene(pt, ctx, moving):
    s = SceneSpec()
    lm = s.add("mat_light", s.add("tex_solid_rgb", 1.0, 1.0, 1.0))
    q = s.add("quad", *B_QUAD, lm)
    axis, a0, a1, tr0, tr1 = B_KEYS
    s.add("world_add_object", s.add("instance_moving", q, axis, a0, a1, tr0, tr1) if moving else s.add("instance", q, axis, a0, tr0))
    s.add("world_build")
    s.camera = default_camera(width=BW, aspect=BW / BH, spp=BSPP, max_depth=1, look_from=(0.0, 0.0, -8.0), look_at=(0.0, 0.0, 0.0), vfov=50.0, focal_length=8.0,
                              defocus_angle=0.0, blur_strength=2.0, env_color=(0.0, 0.0, 0.0))
    gs = pt.Scene(ctx)
    res = s.replay(gs)
    return gs, s.make_camera(pt.Camera, res)


@pytest.mark.parametrize("moving,shutter", [(True, (0.0, 1.0)), (True, (0.25, 0.5)), (False, (0.0, 1.0))], ids=["moving-open", "moving-quarter", "still"])
def test_blur_counts_are_exact(pt, ctx, moving, shutter):
    """max_depth = 1 under a black environment: a sample adds exactly 1 when its camera ray hits the emitter at the pose of its time, so a
    pixel's sum is an integer count that the rule's restatement predicts from pt_camera_probe's rays. Pixels holding a sample within
    1e-9 of an edge of the test are left out (at most 0.5 % of them). At least 10 % of the pixels hold a count strictly between 0 and spp —
    with the shutter open, at least twice as many as the still quad's, whose partial pixels are the pixel filter's (two pixels wide here,
    so that the short shutter reaches the 10 % too). The still case calls nothing this feature added (pt_instance, the camera probe and the
    render only), so it passes without the feature: the restatement and the count check are right on their own."""
    gs, cam = blur_scene(pt, ctx, moving)
    try:
        if moving:
            gs.set_shutter(*shutter)
            assert gs.motion()
        px = np.repeat(np.arange(BW * BH), BSPP)
        rays = gs.camera_probe(cam, BSEED, np.stack([px, np.tile(np.arange(BSPP), BW * BH)], axis=1))
        times = rays[:, 6]
        axis, a0, a1, tr0, tr1 = B_KEYS
        if moving:
            assert shutter[0] <= times.min() and times.max() <= shutter[1] and times.max() - times.min() > 0.9 * (shutter[1] - shutter[0])
            P = MR.poses_at(axis, a0, a1, tr0, tr1, times)
        else:
            P = np.broadcast_to(MR.pose(axis, a0, tr0), (len(times), 8, 3))
        hit, margin = MR.hit_parallelogram_many(*B_QUAD, P, rays[:, 0:3], rays[:, 3:6])
        want = hit.reshape(BH, BW, BSPP).sum(axis=2).astype(np.float64)
        keep = (margin.reshape(BH, BW, BSPP) >= 1e-9).all(axis=2)
        assert (~keep).mean() <= 0.005
        partial = ((want > 0) & (want < BSPP)).mean()
        still = MR.hit_parallelogram_many(*B_QUAD, np.broadcast_to(MR.pose(axis, a0, tr0), (len(times), 8, 3)), rays[:, 0:3], rays[:, 3:6])[0]
        still = still.reshape(BH, BW, BSPP).sum(axis=2)
        partial_still = ((still > 0) & (still < BSPP)).mean()
        print(f"partial pixels: {partial:.4f} (a still quad: {partial_still:.4f}), left out: {(~keep).mean():.5f}")
        assert partial_still > 0.0
        if moving:
            assert partial >= 0.10, partial
            assert shutter != (0.0, 1.0) or partial >= 2.0 * partial_still, (partial, partial_still)
        for spx in (1, 0):                                                  # static and dynamic mode
            acc, st = gs.render(cam, BSEED, 0, BSPP, slots_per_pixel=spx)
            assert st.samples == BW * BH * BSPP
            for c in range(3):
                assert (acc[..., c][keep] == want[keep]).all(), (spx, c, np.abs(acc[..., c] - want)[keep].max())
    finally:
        gs.close()


# ---- 5: refusals and the way back --------------------------------------------------------------------------------------------------------
def test_refusals_and_the_way_back(pt, ctx):
    spec = SceneSpec()
    env = np.array([[[4.0, 3.0, 2.0], [0.5, 0.5, 0.5], [0.25, 0.5, 1.0], [1.0, 1.0, 1.0]], [[0.1, 0.1, 0.1], [0.2, 0.1, 0.0], [0.0, 0.0, 0.0], [0.1, 0.2, 0.1]]], dtype=np.float32)
    tex = spec.add("tex_image_rgbf32", env)
    floor = spec.add("mat_diffuse", spec.add("tex_solid_rgb", 0.6, 0.6, 0.6), -1)
    glass = spec.add("mat_glass", spec.add("tex_solid_rgb", 1.0, 1.0, 1.0), spec.add("tex_solid_f", 0.05), 0.0, 1.5)
    fog = spec.add("mat_medium", 0.05, (0.9, 0.9, 0.9), 0.2)
    spec.add("world_add_object", spec.add("quad", (-8.0, 0.0, -8.0), (0.0, 0.0, 16.0), (16.0, 0.0, 0.0), floor))
    ball = spec.add("sphere", 1.0, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), glass)
    spec.add("world_add_object", spec.add("instance_moving", ball, (0.0, 1.0, 0.0), 0.0, 0.5, (0.0, 0.0, 0.0), (0.5, 0.0, 0.0)))
    tri = np.array([(1.5, 3.0, -0.5), (2.5, 3.0, 0.0), (1.6, 3.0, 0.7)], dtype=np.float32)           # a one-triangle mesh light: exact light sampling can be put in effect
    spec.add("world_add_light", spec.add("mesh", 1.0, tri, np.array([0, 1, 2], dtype=np.uint32), None, None, spec.add("mat_light", spec.add("tex_solid_rgb", 9.0, 8.0, 7.0))))
    spec.add("world_build")
    spec.camera = default_camera(width=16, spp=1, defocus_angle=0.0, env_is_map=1, env_tex=tex)
    gs = pt.Scene(ctx)
    try:
        res = spec.replay(gs)
        cam, glass, fog = spec.make_camera(pt.Camera, res), res[glass], res[fog]
        assert gs.motion()
        features = {
            "environment importance sampling": (lambda: gs.set_env_sampling(0.5), lambda: gs.set_env_sampling(0.0)),
            "participating media or a glass interior": (lambda: gs.set_camera_medium(fog), lambda: gs.set_camera_medium(-1)),
            "exact light sampling": (lambda: gs.set_light_sampling("exact"), lambda: gs.set_light_sampling("reference")),
            "spectral dispersion": (lambda: gs.mat_glass_set_dispersion(glass, 30.0), lambda: gs.mat_glass_set_dispersion(glass, 0.0)),
        }
        for what, (on, off) in features.items():
            on()
            gs.world_build()
            with pytest.raises(pt.PtError, match=f"motion together with {what} is not supported"):
                gs.render(cam, 1, 0, 1)
            off()
            gs.world_build()
            acc, st = gs.render(cam, 1, 0, 1)
            assert st.samples == 16 * 16 and np.isfinite(acc).all()
        # the light probe under exact light sampling refuses moving instances as the render does (its chain walks read the stored poses)
        q = np.array([[0.0, 0.5, 0.0, 0.5]])
        assert gs.light_probe(0, q).shape == (1, 6)
        gs.set_light_sampling("exact")
        with pytest.raises(pt.PtError, match="motion together with exact light sampling is not supported"):
            gs.light_probe(0, q)
        gs.set_light_sampling("reference")
        assert gs.light_probe(0, q).shape == (1, 6)
        for bad in ((-0.1, 0.5), (0.6, 0.5), (0.0, 1.5), (float("nan"), 1.0), (0.0, float("inf"))):
            with pytest.raises(pt.PtError, match="0 <= open <= close <= 1"):
                gs.set_shutter(*bad)
        assert gs.shutter() == (0.0, 1.0)
    finally:
        gs.close()


# ---- 6: boxes ------------------------------------------------------------------------------------------------------------------------------
def test_entry_boxes_hold_every_time(pt, scenes):
    gs, _, rec = scenes("moving")
    t0, _, _ = scenes(("twin", 0.0))
    t1, _, _ = scenes(("twin", 1.0))
    times = np.concatenate([[0.0, 1.0], np.random.default_rng(6).uniform(0.0, 1.0, size=62)])
    n_translate_only = 0
    for e, (points, chain) in enumerate(rec.placements):
        box = gs.entry_box(e)
        for t in times:
            p = points(t)
            for keys in reversed(chain):                                     # innermost instance first; the library's own pose (deterministic sincos):
                p = MR.to_world(pt.motion_pose(*keys, t), p)                   # the tight mesh boxes are unpadded extremes of exactly these points
            assert (p >= box[:3]).all() and (p <= box[3:]).all(), (e, t)
        if len(chain) == 1 and chain[0][1] == chain[0][2] and chain[0][3] != chain[0][4]:
            n_translate_only += 1
            np.testing.assert_array_equal(box, MR.union(t0.entry_box(e), t1.entry_box(e)))
    assert n_translate_only == 1 and len(rec.placements) == 12
    with pytest.raises(Exception, match="out of range"):
        gs.entry_box(len(rec.placements))
