"""Isosurface extraction on the GPU (pt_mesh_isosurface): the device stage against its host twin, byte for byte, on the
shapes of test_iso_cpu.py, at sizes around a wave and a block, on sparse, dense and several-scan-tile grids; then the mesh at work in a
scene (pt_intersect) and on the command line."""
import os
import subprocess

import numpy as np
import pytest

import iso_rule as I
from test_iso_cpu import HI, LO, NORMALS, SHAPES, _radius_bound, _raw, _sphere, assert_closed_manifold, pattern, refusals, same

pytestmark = pytest.mark.gpu


def twin(pt, ctx, v, lo, hi, **kw):
    got = ctx.isosurface(v, lo, hi, **kw)
    same(got, pt.isosurface_host(v, lo, hi, **kw))
    return got


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_matches_the_twin(pt, ctx, name):
    v, lo, hi, kw = SHAPES[name]
    for normals in NORMALS:
        twin(pt, ctx, v, lo, hi, normals=normals, **kw)


@pytest.mark.parametrize("closed", (False, True))
def test_all_corner_patterns(pt, ctx, closed):
    for bits in range(256):
        twin(pt, ctx, pattern(bits, 0.25), LO, HI, iso=0.25, closed=closed, outside=-0.75, normals=NORMALS[bits % 3])


@pytest.mark.parametrize("closed", (False, True))
@pytest.mark.parametrize("nx", (64, 65, 66, 256, 257, 258))
def test_rows_around_a_wave_and_a_block(pt, ctx, nx, closed):
    """nx - 1 cubes in a row: 63 / 64 / 65 and 255 / 256 / 257"""
    rng = np.random.default_rng(nx)
    v = rng.random((2, 2, nx)).astype(np.float32)
    for normals in ("gradient", "smooth"):
        pos, idx, nrm = twin(pt, ctx, v, LO, HI, iso=0.5, closed=closed, outside=0.0, normals=normals)
        assert len(idx) > 3 * nx // 4
    if closed:
        assert_closed_manifold(idx)


def test_sparse(pt, ctx):
    """One non-zero sample in 40^3: long runs of zeros go into both scans"""
    v = np.zeros((40, 40, 40), np.float32)
    v[23, 17, 31] = 1.0
    pos, idx, nrm = twin(pt, ctx, v, LO, HI, iso=0.5)
    assert len(pos) == 14 and len(idx) == 3 * 24                            # the 14 lattice edges at a point, the 24 tetrahedra around it
    assert_closed_manifold(idx)
    twin(pt, ctx, v, LO, HI, iso=0.5, closed=True, normals="smooth")


def test_dense_checkerboard(pt, ctx):
    """17^3 samples of +-1 in a checkerboard: every axis edge crosses, and every cube emits the most triangles it can"""
    k, j, i = np.meshgrid(np.arange(17), np.arange(17), np.arange(17), indexing="ij")
    v = np.where((i + j + k) % 2 == 0, 1.0, -1.0).astype(np.float32)
    per_cube = len(pt.isosurface_host(v[:2, :2, :2], LO, HI, iso=0.0)[1]) // 3
    assert per_cube == max(len(pt.isosurface_host(pattern(b, 0.0), LO, HI, iso=0.0, normals="none")[1]) // 3 for b in range(256))
    for closed in (False, True):
        pos, idx, nrm = twin(pt, ctx, v, LO, HI, iso=0.0, closed=closed, outside=-1.0)
        assert len(idx) >= 3 * per_cube * 16 ** 3


def test_torus_over_several_scan_tiles(pt, ctx):
    lo, hi = (-2.0, -1.5, -1.75), (2.0, 1.5, 1.75)
    v = I.torus_field((96, 80, 72), lo, hi, (0.01, -0.02, 0.03), 1.1, 0.5)
    for kw in (dict(closed=True, outside=-1.0), dict(normals="smooth")):
        pos, idx, nrm = twin(pt, ctx, v, lo, hi, iso=0.0, **kw)
        assert len(pos) - len(idx) // 2 + len(idx) // 3 == 0                # V - E + F with E = 3F / 2 on a closed mesh
    assert np.all(np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0) < 1e-6)


def test_negative_level(pt, ctx):
    rng = np.random.default_rng(5)
    v = (-1.0 - 3.0 * rng.random((9, 11, 13))).astype(np.float32)
    for closed, outside in ((False, 0.0), (True, -10.0), (True, 0.0)):      # outside = 0 > iso: the added layer is inside
        pos, idx, nrm = twin(pt, ctx, v, LO, HI, iso=-2.5, closed=closed, outside=outside)
        assert len(idx) > 0


def test_empty_and_twice_the_same_bytes(pt, ctx):
    ones = np.ones((3, 4, 5), np.float32)
    for kw in (dict(iso=0.5), dict(iso=1.5), dict(iso=1.5, closed=True), dict(iso=0.5, normals="smooth"), dict(iso=1.5, normals="none")):
        pos, idx, nrm = twin(pt, ctx, ones, LO, HI, **kw)
        assert len(pos) == 0 and len(idx) == 0
    v, lo, hi, kw = SHAPES["torus"]
    same(ctx.isosurface(v, lo, hi, **kw), ctx.isosurface(v, lo, hi, **kw))


def test_refusals_on_the_device_path(pt, ctx):
    refusals(pt, lambda *a, **k: _raw(pt, *a, host=False, ctx=ctx.handle, **k))


def test_chain_into_subdivision(pt, ctx):
    v, lo, hi, kw = SHAPES["sphere"]
    pos, idx, nrm = ctx.isosurface(v, lo, hi, **kw)
    got = ctx.subdivide(pos, idx, levels=1, limit=True)
    want = pt.subdivide_host(pos, idx, levels=1, limit=True)
    assert all(g is None if w is None else g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert not got[4].any()


# ---- the result at work: the closed sphere through Scene.mesh, world_build and pt_intersect ------------------------------------------------
@pytest.mark.parametrize("n", ((9, 8, 7), (24, 22, 20)))
def test_rays_meet_the_sphere(pt, ctx, n):
    """Rays aimed at the centre land within the radius bound of the CPU test. That bound was made for vertices; it holds for every point
    of a triangle as well: p = sum w_i v_i has |p|^2 = sum w_i |v_i|^2 - sum_{i<j} w_i w_j |v_i - v_j|^2 >= (r - d)^2 - L^2 / 3 with
    d = L^2 / (8 (r - 2L)) the chord's deviation (a triangle's vertices lie in one lattice cube, so no two are further apart than L), so
    |p| >= (r - d) - L^2 / (6 (r - d)) roughly, and L^2 / (6 (r - d)) <= d, the margin the bound doubles d by, as long as r <= 8L - 3d.
    The 9 x 8 x 7 sphere is larger than its grid and capped (test_iso_cpu.py): there the rays go through the centroids of the triangles
    whose vertices all lie on edges between two samples; the whole sphere of 24 x 22 x 20 is met from random directions."""
    v, c, r, L, h = _sphere(n, LO, HI)
    lower, upper = _radius_bound(r, L)
    assert r <= 8.0 * L - 3.0 * (r - lower) / 2.0
    pos, idx, nrm = twin(pt, ctx, v, LO, HI, iso=0.0, closed=True, outside=-1.0)
    if n == (24, 22, 20):
        d = np.random.default_rng(11).normal(size=(4096, 3))
    else:
        hull_lo, hull_hi = (np.array(LO) + 0.5 * h).astype(np.float32), (np.array(HI) - 0.5 * h).astype(np.float32)
        field = np.all((pos >= hull_lo) & (pos <= hull_hi), axis=1)
        tri = idx.reshape(-1, 3)
        tri = tri[field[tri].all(axis=1)]
        assert len(tri) > 100
        d = pos.astype(np.float64)[tri].mean(axis=1) - c
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    gs = pt.Scene(ctx)
    grey = gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)
    gs.world_add_object(gs.mesh(1.0, pos, idx, nrm, None, grey))
    gs.world_build()
    start = r + 5.0
    rays = np.zeros((len(d), 7))
    rays[:, 0:3], rays[:, 3:6] = c + start * d, -d                          # aimed at the centre from `start` away
    out = gs.intersect(rays)
    gs.close()
    radius = start - out[:, 1]
    print(f"{n}: hits {int(out[:, 0].sum())} of {len(d)}; radius {radius.min():.6f} .. {radius.max():.6f} in [{lower:.6f}, {upper:.6f}]")
    assert np.all(out[:, 0] == 1.0)
    assert radius.min() >= lower and radius.max() <= upper


# ---- the command line: pt_render -s 3 --isosurface ----------------------------------------------------------------------------------------------
def test_cli_isosurface(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    common = [exe, "-q", "-s", "3", "--width", "96", "--spp", "4", "--assets", pt.ASSET_DIR]

    def render(name, *flags):
        png = tmp_path / (name + ".png")
        r = subprocess.run(common + list(flags) + ["--out", str(png)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return pt.load_png_rgb8(str(png))

    plain = render("plain")
    iso = render("iso", "--isosurface", "0.3")
    changed = (plain != iso).any(axis=2)
    print(f"{int(changed.sum())} of {changed.size} pixels differ")
    assert changed.sum() > 0.02 * changed.size                              # the plume stands in the middle of the box, in view
    assert np.array_equal(render("again", "--isosurface", "0.3"), iso)
    assert (render("coarse", "--isosurface", "0.3,24") != iso).any()


def test_cli_isosurface_refusals(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    out = tmp_path / "bad.png"
    for flags, text in ((("--isosurface", "0.3", "--smoke", "1"), "--smoke"), (("--isosurface", "0.3", "--fog", "0.1"), "--fog"), (("--isosurface", "x"), "ISO"),
                        (("--isosurface", "0.3,1"), "GRID_N"), (("--isosurface", "0.3,24.5"), "GRID_N"), (("--isosurface", "0.3,24,1"), "ISO")):
        r = subprocess.run([exe, "-q", "-s", "3", "--width", "32", "--spp", "1", "--assets", pt.ASSET_DIR, *flags, "--out", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and text in r.stderr, (flags, r.stderr)
        assert not out.exists()
    r = subprocess.run([exe, "-q", "-s", "3", "--width", "32", "--spp", "1", "--assets", pt.ASSET_DIR, "--isosurface", "5", "--out", str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "does not cross" in r.stderr and not out.exists()      # the plume never reaches 5
