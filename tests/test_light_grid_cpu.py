"""The light grid (pt_scene_set_punctual_selection kind 1) without a device: the ABI symbols, bindings and the header's
text, the host twins of the build kernel's and K3's functions against the numpy restatement of the rule (tests/light_grid_rule.py) bit for
bit, the properties of every row, the variance the rule predicts for a row of lamps by enumeration, and the CLI's refusals."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import light_grid_rule as LG

NEW_SYMBOLS = ("pt_scene_set_punctual_selection", "pt_scene_punctual_selection", "pt_scene_set_punctual_grid", "pt_scene_punctual_grid",
               "pt_punctual_grid_row", "pt_punctual_grid_select")
BOX = np.array([-2.0, 0.0, -1.0, 2.0, 3.0, 4.0])
DIMS = (4, 3, 5)


def test_symbols_bindings_and_header(pt):
    header = open(os.path.join(pt.REPO_ROOT, "include", "pt_amd.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym in pt.ABI_SYMBOLS and hasattr(pt.lib, sym) and sym + "(" in header, sym
        assert getattr(pt.lib, sym).argtypes is not None, sym
    assert len(pt.lib.pt_punctual_probe.argtypes) == 5 and len(pt.lib.pt_scene_set_punctual_grid.argtypes) == 5
    assert len(pt.lib.pt_punctual_grid_row.argtypes) == 6 and len(pt.lib.pt_punctual_grid_select.argtypes) == 8
    for method in ("set_punctual_selection", "punctual_selection", "set_punctual_grid", "punctual_grid"):
        assert hasattr(pt.Scene, method), method
    assert callable(pt.punctual_grid_row) and callable(pt.punctual_grid_select)
    # the rule, as the issue states it; the two older sections are still there
    for text in ("(iz * ny + iy) * nx + ix", "s = (hi - lo) / (double)n_axis", "rc2 = (hx * hx + hy * hy) + hz * hz", "Y = (I_r + I_g) + I_b",
                 "w = Y / (dmin2 + rc2)", "c_far = cos_o * ca - so * sa", "cos_o > -ca && c_m < c_far - 1e-9", "p_k = 0.875 *", "0.125 / (double)n",
                 "stored as exactly 1.0", "the smallest index with u < C[k]", "pm = f * p", "below 2e-12", "cells * n <= 2^25", "clamp(ceil(R * ext / ext_max), 1, R)",
                 "which 2: in = n x point.xyz", "which 3: in = n x (cell, k)", "pm = f / (double)n", "Selection is uniform, not by power", "The selector draw r is READ"):
        assert text in header, text
    hpp = open(os.path.join(os.path.dirname(pt.__file__), "host", "pt.hpp")).read()
    for text in ("punctual_selection", "punctual_grid", "pt_scene_set_punctual_selection("):
        assert text in hpp, text
    for doc, texts in (("INTEGRATION.md", ("pt_scene_set_punctual_selection",)), ("README.md", ("--punctual-selection", "pt_scene_set_punctual_selection")),
                       ("DESIGN.md", ("## 26", "No light tree", "No visibility in the importance", "pt_scene_set_punctual_selection"))):
        body = open(os.path.join(pt.REPO_ROOT, doc)).read()
        for text in texts:
            assert text in body, (doc, text)


def test_refusals_without_a_scene(pt):
    lib = pt.lib
    assert lib.pt_scene_set_punctual_selection(None, 1) == -1 and b"null scene" in lib.pt_last_error()
    assert lib.pt_scene_punctual_selection(None) == -1
    assert lib.pt_scene_set_punctual_grid(None, 0, 0, 0, None) == -1 and b"null scene" in lib.pt_last_error()
    assert lib.pt_scene_punctual_grid(None, None, None) == -1
    recs = lights(3)
    good = pt.punctual_grid_row(recs, BOX, DIMS, 59)
    assert good.shape == (3,) and good[-1] == 1.0
    nan = float("nan")
    for box, dims, cell, word in ((BOX, (0, 3, 5), 0, "1..64"), (BOX, (4, 65, 5), 0, "1..64"), (BOX, DIMS, 60, "no such cell"),
                                  ([-2, 0, -1, 2, nan, 4], DIMS, 0, "finite"), ([-2, 0, -1, 2, float("inf"), 4], DIMS, 0, "finite"), ([-2, 3.5, -1, 2, 3, 4], DIMS, 0, "hi >= lo")):
        with pytest.raises(pt.PtError, match=word):
            pt.punctual_grid_row(recs, box, dims, cell)
    with pytest.raises(pt.PtError, match="1..2048"):
        pt.punctual_grid_row(np.zeros((0, 16)), BOX, DIMS, 0)
    with pytest.raises(pt.PtError, match="1..2048"):
        pt.punctual_grid_row(np.zeros((2049, 16)), BOX, DIMS, 0)
    bad = recs.copy()
    bad[1, 0] = 3.0
    with pytest.raises(pt.PtError, match="kind"):
        pt.punctual_grid_row(bad, BOX, DIMS, 0)
    d = (C.c_uint32 * 3)(*DIMS)
    b = (C.c_double * 6)(*BOX)
    assert lib.pt_punctual_grid_row(None, 3, b, d, 0, (C.c_double * 3)()) == -1 and lib.pt_punctual_grid_row(recs.ctypes.data, 3, None, d, 0, (C.c_double * 3)()) == -1
    assert lib.pt_punctual_grid_row(recs.ctypes.data, 3, b, None, 0, (C.c_double * 3)()) == -1 and lib.pt_punctual_grid_row(recs.ctypes.data, 3, b, d, 0, None) == -1
    assert lib.pt_punctual_grid_select(b, d, None, 3, b, b, 1, (C.c_double * 3)()) == -1 and b"null" in lib.pt_last_error()
    with pytest.raises(pt.PtError, match="table is"):
        pt.punctual_grid_select(BOX, DIMS, np.ones((59, 3)), [[0.0, 0.0, 0.0]], [0.5])


# ---- the lists -----------------------------------------------------------------------------------------------------------------------------
def rec(kind, pos, axis, I, ci=0.0, co=0.0):
    a = np.asarray(axis, dtype=np.float64)
    n = math.sqrt(float(a @ a))
    return np.array([kind, *pos, *(a / n if n > 0.0 else a), *I, ci, co, 0.0, 0.0, 0.0, 0.0], dtype=np.float64)


def cosd(deg):
    return math.cos(math.radians(deg))


def lights(n, box=BOX, dims=DIMS, seed=2610):
    """n records: the first ten are the issue's cases — a light inside a cell, on a cell corner and far outside the box, spots aimed at, across
    and away from the box, a spot with outer_deg near 0 and one near 180, a light of colour (0, 0, 0) — and all three kinds are among the
    first three; the rest are random lights of all kinds in and around the box."""
    lo, hi = box[:3], box[3:]
    ctr, ext = (lo + hi) * 0.5, hi - lo
    step = ext / np.asarray(dims, dtype=np.float64)
    out_pos = ctr + np.array([2.5, 0.3, 0.2]) * np.maximum(ext, 1.0)
    special = [rec(0, lo + ext * np.array([0.31, 0.77, 0.13]), (0, 0, 0), (3.0, 2.0, 1.0)),                      # inside a cell
               rec(1, out_pos, ctr - out_pos, (9.0, 8.0, 7.0), cosd(2.0), cosd(4.0)),                            # a spot aimed at the box
               rec(2, (0, 0, 0), (0.3, -1.0, 0.2), (3.0, 2.5, 2.0)),                                             # a sun
               rec(0, lo + step * np.array([1.0, 1.0, 2.0]), (0, 0, 0), (1.0, 1.0, 1.0)),                        # on a cell corner
               rec(1, out_pos, out_pos - ctr, (9.0, 8.0, 7.0), cosd(10.0), cosd(20.0)),                          # a spot aimed away
               rec(0, (1e4, -3e3, 2e4), (0, 0, 0), (5e6, 5e6, 5e6)),                                             # far outside
               rec(1, out_pos, np.cross(ctr - out_pos, (0.0, 1.0, 0.1)), (4.0, 4.0, 4.0), cosd(5.0), cosd(12.0)),   # a spot across
               rec(1, lo + ext * np.array([0.5, 0.9, 0.5]), (0.1, -1.0, 0.05), (6.0, 6.0, 6.0), cosd(1e-4), cosd(1e-3)),   # outer_deg near 0
               rec(1, lo + ext * np.array([0.2, 0.5, 0.8]), (0.0, 1.0, 0.0), (2.0, 2.0, 2.0), cosd(90.0), cosd(179.9)),    # outer_deg near 180
               rec(0, lo + ext * np.array([0.6, 0.4, 0.6]), (0, 0, 0), (0.0, 0.0, 0.0))]                         # black
    rng = np.random.default_rng(seed)
    out = list(special[:n])
    while len(out) < n:
        kind = int(rng.integers(0, 3))
        pos = ctr + rng.uniform(-1.5, 1.5, 3) * np.maximum(ext, 1.0)
        outer = rng.uniform(2.0, 120.0)
        out.append(rec(kind, pos, rng.normal(size=3), rng.uniform(0.0, 10.0, 3), cosd(outer * rng.uniform(0.0, 1.0)), cosd(outer)))
    return np.stack(out)


FLAT_BOX = np.array([-2.0, 1.0, -1.0, 2.0, 1.0, 4.0])                     # an axis of extent 0
GRIDS = [("one cell", BOX, (1, 1, 1)), ("4x3x5", BOX, DIMS), ("flat", FLAT_BOX, (4, 2, 3))]


def host_table(pt, recs, box, dims):
    return np.stack([pt.punctual_grid_row(recs, box, dims, c) for c in range(dims[0] * dims[1] * dims[2])])


def assert_rows(T, n):
    assert (np.diff(T, axis=1) >= 0.0).all() and (T[:, -1] == 1.0).all() and (T[:, 0] > 0.0).all()
    assert (LG.probabilities(T) >= 0.125 / n * (1.0 - 1e-12)).all()


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 2048])
def test_host_rows_equal_the_rule_bit_for_bit(pt, n):
    grids = GRIDS if n < 2048 else [("2x2x2", BOX, (2, 2, 2))]
    for name, box, dims in grids:
        recs = lights(n, box, dims)
        if n >= 3:
            assert set(recs[:3, 0]) == {0.0, 1.0, 2.0}
        want = LG.table(recs, box, dims)
        got = host_table(pt, recs, box, dims)
        assert got.tobytes() == want.tobytes(), (name, n, np.argwhere(got != want)[:5])
        assert_rows(got, n)
        if n >= 64 and name == "4x3x5":
            w = LG.weights(recs, box, dims)
            spots = (recs[:, 0] == 1.0) & (recs[:, 7:10].sum(axis=1) > 0.0)
            culled = (w[:, spots] == 0.0)
            assert culled.any() and not culled.all() and culled.any(axis=0).sum() >= 5                 # the cone cull fires for some cells, not for all
            assert (w[:, 4] == 0.0).all() and (w[:, 1] > 0.0).any() and (w[:, 1] == 0.0).any()          # aimed away: every cell culled; aimed at: some
            assert (w[:, 7] == 0.0).sum() >= 40 and (w[:, 7] > 0.0).any() and (w[:, 8] > 0.0).all()     # outer near 0: a few cells; near 180: every cell
            assert (w[:, 9] == 0.0).all()                                                                # the black light: the floor alone
            p = LG.probabilities(got)
            np.testing.assert_allclose(p[:, 9], 0.125 / n, rtol=1e-9)
            assert p[:, 0].argmax() == LG.cell_of(box, dims, recs[0, 1:4])[0]                            # the light inside a cell counts most there


def test_uniform_rows(pt):
    """a list whose colours are all zero (W = 0), and a zero-size cell that holds a light (W is not finite): uniform rows"""
    recs = lights(7)
    recs[:, 7:10] = 0.0
    for name, box, dims in GRIDS:
        got = host_table(pt, recs, box, dims)
        assert got.tobytes() == LG.table(recs, box, dims).tobytes()
        want = np.cumsum(np.full(7, 1.0 / 7.0))
        want[-1] = 1.0
        assert (got == want[None, :]).all(), name
    point = np.array([0.5, 1.0, -0.25])
    box = np.concatenate([point, point])
    for colour in ((2.0, 2.0, 2.0), (0.0, 0.0, 0.0)):                      # Y / 0 = inf, 0 / 0 = NaN
        recs = np.stack([rec(0, point, (0, 0, 0), colour), rec(0, point + 1.0, (0, 0, 0), (1.0, 1.0, 1.0)), rec(2, (0, 0, 0), (0, -1, 0), (1.0, 1.0, 1.0))])
        w = LG.weights(recs, box, (1, 1, 1))
        assert not np.isfinite(w[0, 0])
        got = pt.punctual_grid_row(recs, box, (1, 1, 1), 0)
        assert got.tobytes() == LG.table(recs, box, (1, 1, 1))[0].tobytes()
        assert (got == np.array([1.0 / 3.0, 1.0 / 3.0 + 1.0 / 3.0, 1.0])).all()


def test_automatic_dims():
    assert LG.auto_dims([0, 0, 0, 16, 4, 1], 8) == (16, 4, 1) and LG.auto_dims([0, 0, 0, 1, 1, 1], 2048) == (16, 16, 16)
    assert LG.auto_dims([0, 0, 0, 2, 0, 1.01], 4) == (16, 1, 9) and LG.auto_dims([1, 1, 1, 1, 1, 1], 4) == (1, 1, 1)
    assert LG.auto_dims([0, 0, 0, 1, 1, 1], 2048) == (16, 16, 16) and 16 ** 3 * 2048 <= LG.CAP < 32 ** 3 * 2048


def test_host_select_equals_the_rule(pt):
    n, m = 64, 1 << 16
    recs = lights(n)
    T = LG.table(recs, BOX, DIMS)
    rng = np.random.default_rng(97)
    lo, hi = BOX[:3], BOX[3:]
    pts = rng.uniform(lo - 0.5, hi + 0.5, (m, 3))                         # inside and outside
    a, b, _, _ = LG.cell_geometry(BOX, DIMS)
    faces = np.concatenate([a, b])[rng.integers(0, 2 * len(a), 4096)]      # on cell faces: coordinates that are some cell's a or b, the box's faces included
    pts[:4096] = np.where(rng.random((4096, 3)) < 0.7, faces, pts[:4096])
    pts[4096:4104] = [lo, hi, lo - 1e-300, hi + 1e-9, [np.inf, 0.0, 0.0], [-np.inf, 1.0, 1.0], [np.nan, np.nan, np.nan], [0.0, np.nan, 5.0]]
    u = rng.random(m)
    u[:2048] = T[rng.integers(0, len(T), 2048), rng.integers(0, n - 1, 2048)]       # exactly on a boundary: u = C[j] belongs to j + 1
    u[2048:2052] = [0.0, np.nextafter(1.0, 0.0), 0.5, 2.0 ** -53]
    want = LG.select(BOX, DIMS, T, pts, u)
    got = pt.punctual_grid_select(BOX, DIMS, T, pts, u)
    assert (got[:, 0] == want[0]).all() and (got[:, 1] == want[1]).all() and got[:, 2].tobytes() == want[2].tobytes()
    cell, k = got[:, 0].astype(int), got[:, 1].astype(int)
    assert len(np.unique(cell)) == 60 and len(np.unique(k)) == n
    below = np.where(k > 0, T[cell, np.maximum(k - 1, 0)], 0.0)
    assert (below <= u).all() and (u < T[cell, k]).all()
    assert (got[:, 2] >= 0.125 / n * (1.0 - 1e-12)).all()
    assert cell[4096 + 6] == 0 and cell[4096 + 1] == 59                    # a NaN takes cell 0; the box's far corner the last cell


def test_variance_the_rule_predicts_for_a_row_of_lamps():
    """32 equal lamps over a Lambert floor: the exact per-sample variance of the punctual estimator, sum_k c_k^2 / (f p_k) - S^2 with c_k = e E_k,
    under the grid's p against the uniform p_k = 1 / n, at 20 000 fixed-seed floor points. No rendering, no random draws of the estimator."""
    n, f = 32, 0.5
    recs = np.stack([rec(0, (-8.0 + 16.0 * (k + 0.5) / n, 0.4, 0.0), (0, 0, 0), (1.0, 1.0, 1.0)) for k in range(n)])
    box, dims = [-8.0, 0.0, -1.0, 8.0, 0.4, 1.0], (16, 1, 2)
    T = LG.table(recs, box, dims)
    rng = np.random.default_rng(20000)
    x = np.stack([rng.uniform(-8.0, 8.0, 20000), np.zeros(20000), rng.uniform(-1.0, 1.0, 20000)], axis=1)
    L = recs[None, :, 1:4] - x[:, None, :]
    d2 = (L * L).sum(axis=2)
    cos = L[:, :, 1] / np.sqrt(d2)
    c = (cos * (1.0 / math.pi)) * (1.0 / d2)                               # e * E_k: Lambert's |cos| * (albedo / pi), albedo 1, times I / d2, I = 1
    p = LG.probabilities(T)[LG.cell_of(box, dims, x)]
    v_grid, v_uni = LG.variance(c, p, f), LG.variance(c, np.full_like(p, 1.0 / n), f)
    best = LG.variance(c, c / c.sum(axis=1, keepdims=True), f)
    mean_ratio, max_ratio = v_grid.mean() / v_uni.mean(), (v_grid / v_uni).max()
    print(f"variance ratio grid / uniform: mean {mean_ratio:.4f}, pointwise max {max_ratio:.4f}; a perfect choice {best.mean() / v_uni.mean():.4f}")
    assert mean_ratio < 0.2 and max_ratio < 0.25


def test_cli_refuses_bad_selections(pt):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    run = lambda *a: subprocess.run([exe, *a], capture_output=True, text=True, timeout=60)
    assert "--punctual-selection uniform|grid[,NX,NY,NZ]" in run("--help").stdout
    for bad in ("tree", "grid,4", "grid,4,4", "grid,0,4,4", "grid,4,4,65", "grid,4,4,x", "uniform,4,4,4", "grid,4,4,4,4", ""):
        p = run("--punctual-selection", bad)
        assert p.returncode == 2 and p.stderr.strip(), bad
