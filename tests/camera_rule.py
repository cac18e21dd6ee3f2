"""The camera projections' rule (pt_scene_set_projection in include/pt_amd.h) restated in numpy from the header's text,
for the projection tests. The draws come from sampler_rule (independent_u64 / sobol_u64), the frame vectors from pt_camera_init (the
rule names them as its inputs), and sine and cosine from the oracle's deterministic-math binding (oracle_py.detmath 3 / 4, one
scalar call per value), which has every elementary function the rule needs — so values can be compared with the device bit for bit.
numpy's +, -, *, / and sqrt on float64 are IEEE operations with one rounding each, as the rule asks."""
import numpy as np

import sampler_rule as R

KINDS = {"perspective": 0, "orthographic": 1, "fisheye": 2, "panorama": 3}
PI = np.pi


def _det(which, x):
    import oracle_py

    x = np.asarray(x, dtype=np.float64)
    return np.array([oracle_py.detmath(which, float(v)) for v in x.reshape(-1)], dtype=np.float64).reshape(x.shape)


def det_sin(x):
    return _det(3, x)


def det_cos(x):
    return _det(4, x)


def _normalize(v):
    """Ray::new's normalisation: v * (1 / length), the dot product summed left to right."""
    d = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
    return v * (1.0 / np.sqrt(d))[..., None]


class Draws:
    """The sample's stream from draw 0 under either sampler, with the Sobol sampler's pair alignment of two-value draws."""

    def __init__(self, seed, pixels, samples, sobol):
        self.f = R.sobol_u64 if sobol else R.independent_u64
        self.sobol, self.seed = sobol, seed
        self.p, self.s = np.asarray(pixels, dtype=np.uint64), np.asarray(samples, dtype=np.uint64)
        self.draw = 0

    def pair(self, used=True):
        if self.sobol:
            self.draw = (self.draw + 1) & ~1
        d = self.draw
        self.draw += 2
        if not used:
            return None
        return R.unit(self.f(self.seed, self.p, self.s, d)), R.unit(self.f(self.seed, self.p, self.s, d + 1))

    def single(self, used=True):
        d = self.draw
        self.draw += 1
        return R.unit(self.f(self.seed, self.p, self.s, d)) if used else None


def _offsets(u0, u1):
    radius, angle = np.sqrt(u0), u1 * 2.0 * PI
    return radius * det_cos(angle), radius * det_sin(angle)


def lens_radius(defocus_angle, focal_length):
    return np.tan((defocus_angle / 2.0) * (PI / 180.0)) * focal_length


def camera_rays(kind, frame, height, cam, seed, pixels, samples, sobol, motionless=False):
    """The rays of (pixel, sample) pairs (two arrays of one shape) under projection `kind`. frame, height: pt_camera_init's output;
    cam: a mapping or object with image_width, blur_strength, focal_length, defocus_angle, vfov, look_from. motionless: nothing in the
    (built) scene moves, so the time draw is made by index only and time is 0. Returns (origin (n, 3), direction (n, 3), time (n,),
    draws consumed)."""
    g = (lambda k: cam[k]) if isinstance(cam, dict) else (lambda k: getattr(cam, k))
    kind = KINDS.get(kind, kind)
    W, H, F = float(g("image_width")), float(height), float(g("focal_length"))
    pixels = np.asarray(pixels, dtype=np.int64).reshape(-1)
    samples = np.asarray(samples, dtype=np.int64).reshape(-1)
    rows, cols = np.divmod(pixels, int(W))
    center = np.array([float(x) for x in g("look_from")])
    forward, right, up = (np.asarray(frame[k], dtype=np.float64) for k in ("forward", "right", "up"))
    p00, du, dv = (np.asarray(frame[k], dtype=np.float64) for k in ("pixel00", "pixel_du", "pixel_dv"))
    radius = lens_radius(float(g("defocus_angle")), F)
    lens = radius != 0.0
    dof_right, dof_up = right * radius, up * radius

    st = Draws(seed, pixels, samples, sobol)
    bx, by = _offsets(*st.pair())
    bx, by = bx * float(g("blur_strength")), by * float(g("blur_strength"))
    px = py = None
    if lens:
        px, py = _offsets(*st.pair())
    else:
        st.pair(used=False)
    time = np.zeros(len(pixels)) if motionless else st.single()
    if motionless:
        st.single(used=False)
    fy, fx = rows + bx, cols + by

    if kind in (0, 1):
        S = p00 + dv * fy[:, None] + du * fx[:, None]
    if kind == 0:
        O = np.broadcast_to(center, S.shape)
        if lens:
            O = O + dof_right * px[:, None] + dof_up * py[:, None]
        w = S - O
    elif kind == 1:
        O = S + forward * F
        if lens:
            O = (O + dof_right * px[:, None]) + dof_up * py[:, None]
        w = S - O
    elif kind == 2:
        th = (float(g("vfov")) * (PI / 180.0)) / 2.0
        xn, yn = (2.0 * (fx + 0.5) - W) / H, (H - 2.0 * (fy + 0.5)) / H
        rho = np.sqrt(xn * xn + yn * yn)
        theta = np.minimum(rho * th, PI)
        s, c = det_sin(theta), det_cos(theta)
        with np.errstate(invalid="ignore", divide="ignore"):
            a = np.where(rho > 0.0, s / rho, 0.0)
        w = (right * (xn * a)[:, None] + up * (yn * a)[:, None]) - forward * c[:, None]
        O = np.broadcast_to(center, w.shape)
    elif kind == 3:
        phi = -PI + ((2.0 * PI) * (fx + 0.5)) / W
        theta = np.minimum(np.maximum((PI * (fy + 0.5)) / H, 0.0), PI)
        st_, ct = det_sin(theta), det_cos(theta)
        sp, cp = det_sin(phi), det_cos(phi)
        w = np.stack([st_ * cp, ct, st_ * sp], axis=1)
        O = np.broadcast_to(center, w.shape)
    else:
        raise ValueError(kind)
    return np.array(O), _normalize(w), time, st.draw


def fisheye_refused(width, height, vfov):
    """The fisheye refusals of the rule: vfov not finite or not > 0, or an image circle that does not cover the frame."""
    if not np.isfinite(vfov) or not vfov > 0.0:
        return True
    th = (vfov * (PI / 180.0)) / 2.0
    a = float(width) / float(height)
    return bool(np.sqrt(a * a + 1.0) * th > PI)


def environment_texel(d, W, H):
    """The texel (i, j) the environment lookup (camera.rs:140-151, tex_image's clamps) reads for unit directions d (n, 3), with libm's
    acos / atan2: away from texel borders the last bits do not matter."""
    theta = np.arccos(np.clip(d[:, 1], -1.0, 1.0))
    phi = np.arctan2(d[:, 2], d[:, 0])
    u = np.clip((phi + PI) / (2.0 * PI), 0.0, 1.0)
    v = 1.0 - np.clip(1.0 - theta / PI, 0.0, 1.0)
    return np.minimum((u * W).astype(np.int64), W - 1), np.minimum((v * H).astype(np.int64), H - 1)
