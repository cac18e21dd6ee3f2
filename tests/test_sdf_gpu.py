"""Mesh voxelisation on the GPU (pt_mesh_sdf): the device stage against its host twin, byte for byte, on every shape and
mode of test_sdf_cpu.py; at triangle counts around a lane tile (64) and an LDS tile (256); on one brick, ragged bricks and rows longer
than a wave; at both extremes of the rasteriser; on spot with and without a band (the twin has no brick cull: this is the cull's proof
on real data); then the grid at work in a medium, through isosurface extraction, under rays, and on the command line."""
import os
import subprocess

import numpy as np
import pytest

import iso_rule as I
import sdf_rule as S
from test_iso_cpu import assert_closed_manifold
from test_sdf_cpu import _raw, refusals, same, shapes

pytestmark = pytest.mark.gpu

MODES = (dict(), dict(negate=True), dict(fill="odd"), dict(what="distance"), dict(what="occupancy"), dict(what="occupancy", fill="odd"), dict(what="density", ramp=0.25),
         dict(band=0.2), dict(what="distance", band=0.07))


def twin(pt, ctx, pos, idx, dims, lo, hi, **kw):
    got = ctx.mesh_sdf(pos, idx, dims, lo, hi, **kw)
    same(got, pt.mesh_sdf_host(pos, idx, dims, lo, hi, **kw))
    return got


@pytest.mark.parametrize("name", ("tetrahedron", "octahedron", "cube", "torus", "sphere"))
def test_shape_matches_the_twin(pt, ctx, name):
    for kw in MODES:
        twin(pt, ctx, *shapes(pt)[name], **kw)


def test_bodies_of_the_cpu_file(pt, ctx):
    """Ties on sample centres, inside out, the shell, the overlap, degenerate triangles, the three box placements, the open quad"""
    dims, lo, hi = (8, 8, 8), (0.0, 0.0, 0.0), (4.0, 4.0, 4.0)
    cube = S.cube((0.75, 1.25, 0.25), (2.75, 3.25, 2.25))
    occ = twin(pt, ctx, *cube, dims, lo, hi, what="occupancy")
    assert occ.sum() == 4 * 4 * 4                                               # the half-open [c0, c1)^3
    twin(pt, ctx, *cube, dims, lo, hi)
    twin(pt, ctx, *S.octahedron((1.75, 2.25, 1.75), 1.5), dims, lo, hi)
    pos, idx = cube
    for fill in ("nonzero", "odd"):
        same(twin(pt, ctx, pos, S.flipped(idx), dims, lo, hi, fill=fill), ctx.mesh_sdf(pos, idx, dims, lo, hi))
    dims, lo, hi = (10, 9, 8), (0.0, 0.0, 0.0), (5.0, 4.5, 4.0)
    outer, inner = S.cube((0.6, 0.6, 0.6), (4.4, 3.9, 3.4)), S.cube((1.6, 1.6, 1.6), (3.4, 2.9, 2.4))
    overlap = S.merged(S.cube((0.6, 0.6, 0.6), (3.1, 3.1, 3.1)), S.cube((1.9, 1.4, 0.9), (4.4, 3.9, 3.4)))
    for mesh in (S.merged(outer, (inner[0], S.flipped(inner[1]))), overlap):
        for kw in (dict(), dict(fill="odd"), dict(what="occupancy", fill="odd")):
            twin(pt, ctx, *mesh, dims, lo, hi, **kw)
    assert (ctx.mesh_sdf(*overlap, dims, lo, hi, what="occupancy") != ctx.mesh_sdf(*overlap, dims, lo, hi, what="occupancy", fill="odd")).any()
    pos, idx, dims, lo, hi = shapes(pt)["sphere"]
    extra = np.concatenate([pos, np.array([[0.125, 0.25, 0.375], [0.25, 0.5, 0.75], [0.5, 1.0, 1.5]], np.float32)])
    n = len(pos)
    junk = np.array([n, n + 1, n + 2, 5, 5, 9, 7, 3, 7, n + 1, n + 1, n + 1], np.uint32)
    mixed = np.concatenate([idx[:30], junk[:6], idx[30:], junk[6:]])
    for kw in (dict(), dict(what="density", ramp=0.3)):
        same(twin(pt, ctx, extra, mixed, dims, lo, hi, **kw), ctx.mesh_sdf(pos, idx, dims, lo, hi, **kw))
    pos, idx = S.octahedron((0.1, 0.2, 0.3), 2.0)
    for lo, hi in (((3.0, 2.5, 4.0), (4.5, 3.5, 5.5)), ((-0.2, 0.0, 0.1), (0.3, 0.4, 0.5)), ((-0.5, -3.0, 0.2), (3.5, 1.0, 2.9))):
        for kw in (dict(), dict(what="density", ramp=0.5), dict(band=0.3)):
            twin(pt, ctx, pos, idx, (7, 6, 5), lo, hi, **kw)
    quad = np.array([[0, 0, 0.5], [1, 0, 0.5], [1, 1, 0.5], [0, 1, 0.5]], np.float32)
    twin(pt, ctx, quad, np.array([0, 1, 2, 0, 2, 3], np.uint32), (6, 7, 5), (-0.5, -0.6, -0.2), (1.6, 1.5, 1.3), what="distance")


@pytest.mark.parametrize("count", (1, 63, 64, 65, 255, 256, 257, 600))
def test_triangle_counts(pt, ctx, count):
    """A lane tile of the cull is 64 triangles, an LDS tile 256: the torus cut to length (an open mesh: what = 1)"""
    pos, idx, dims, lo, hi = shapes(pt)["torus"]
    assert len(idx) // 3 >= 600
    for kw in (dict(what="distance"), dict(what="distance", band=0.4)):
        twin(pt, ctx, pos, idx[:3 * count], dims, lo, hi, **kw)


@pytest.mark.parametrize("dims", ((2, 2, 2), (4, 4, 4), (5, 3, 7), (9, 6, 11), (65, 4, 4), (4, 4, 130), (40, 36, 33)))
def test_grids(pt, ctx, dims):
    """One brick, ragged bricks, rows longer than a wave (the suffix pass), more bricks than one block takes"""
    pos, idx, _, lo, hi = shapes(pt)["torus" if dims == (40, 36, 33) else "sphere"]   # whole closed meshes: the signed modes
    for kw in (dict(), dict(what="occupancy"), dict(what="density", ramp=0.25), dict(band=0.3)):
        got = twin(pt, ctx, pos, idx, dims, lo, hi, **kw)
    assert (got < 0).any() and ((got > 0).any() or dims == (2, 2, 2))             # (the eight centres of 2 x 2 x 2 lie outside the sphere)


def test_past_the_launch_caps(pt, ctx):
    """Every kernel walks its work by stride from a grid of at most 4096 blocks. 68 x 132 x 132 samples are 18 513 bricks (k_sdf_dist takes
    four a block: 16 384 fit one pass), 17 424 rows (k_sdf_rows: four a block) and 1.18 M samples (k_sdf_occupancy: 1 M fit); a torus of
    more than 16 384 triangles takes k_sdf_raster (four triangles a block) round as well. A dozen triangles keep the twin fast."""
    pos, idx, _, lo, hi = shapes(pt)["cube"]
    dims = (68, 132, 132)
    assert 17 * 33 * 33 > 4 * 4096 and 132 * 132 > 4 * 4096 and 68 * 132 * 132 > 256 * 4096
    for kw in (dict(), dict(what="occupancy"), dict(what="density", ramp=0.25), dict(band=0.1)):
        got = twin(pt, ctx, pos, idx, dims, lo, hi, **kw)
    assert (got > 0).any() and (got < 0).any()
    tlo, thi = (-2.0, -1.0, -2.0), (2.0, 1.0, 2.0)
    tp, ti, _ = pt.isosurface_host(I.torus_field((40, 20, 40), tlo, thi, (0.05, 0.02, -0.03), 1.2, 0.45), tlo, thi, iso=0.0, closed=True, outside=-1.0, normals="none")
    assert len(ti) // 3 > 4 * 4096
    occ = twin(pt, ctx, tp, ti, (13, 9, 12), (-2.1, -1.1, -2.2), (2.2, 1.2, 2.1), what="occupancy")
    assert 0 < occ.sum() < occ.size
    twin(pt, ctx, tp, ti, (7, 5, 6), (-2.1, -1.1, -2.2), (2.2, 1.2, 2.1))


def test_long_row_through_many_crossings(pt, ctx):
    """A row of 300 samples through five nested shells: the suffix pass carries a winding across chunks of 64"""
    meshes, sign = [], 1
    for r in (1.45, 1.2, 0.9, 0.6, 0.3):
        p, i = S.cube((-r, -0.5 * r, -0.4 * r), (r, 0.5 * r, 0.4 * r))
        meshes.append((p, i if sign > 0 else S.flipped(i)))
        sign = -sign
    pos, idx = S.merged(*meshes)
    for fill in ("nonzero", "odd"):
        got = twin(pt, ctx, pos, idx, (300, 5, 5), (-1.5, -0.8, -0.75), (1.5, 0.8, 0.75), what="occupancy", fill=fill)
    assert 0 < got.sum() < got.size and np.count_nonzero(np.diff(got[2, 2])) == 10


def test_raster_extremes(pt, ctx):
    """A few triangles that cover thousands of columns each; many triangles that cover a column or none"""
    pos, idx, _, lo, hi = shapes(pt)["cube"]
    got = twin(pt, ctx, pos, idx, (64, 64, 8), lo, hi)
    assert (got > 0).sum() > 5000
    twin(pt, ctx, pos, idx, (64, 64, 8), lo, hi, what="occupancy")
    pos, idx, _, lo, hi = shapes(pt)["torus"]
    twin(pt, ctx, pos, idx, (12, 12, 12), lo, hi)
    twin(pt, ctx, pos, idx, (12, 12, 12), lo, hi, what="occupancy")


@pytest.fixture(scope="module")
def spot(pt):
    pos, idx, uv = pt.load_obj(os.path.join(pt.ASSET_DIR, "spot.obj"))
    dims, lo, hi = pt.mesh_fit_grid(pos, 40, 2.0)
    return pos, idx, dims, lo, hi


def test_spot_cull_against_no_cull(pt, ctx, spot):
    """The twin tests every triangle its own point cannot rule out; the device culls by brick. spot, about 24 x 40 x 40"""
    pos, idx, dims, lo, hi = spot
    assert dims[2] == 40 and 20 <= dims[0] <= 30 and 34 <= dims[1] <= 40
    h = (hi[0] - lo[0]) / dims[0]
    depth = twin(pt, ctx, pos, idx, dims, lo, hi)
    banded = twin(pt, ctx, pos, idx, dims, lo, hi, band=3.0 * h)
    b = np.float32(3.0 * h)
    same(banded, np.clip(depth, -b, b))
    same(ctx.mesh_sdf(pos, idx, dims, lo, hi), depth)                           # the same call twice: the same bytes
    cell = float(np.prod((hi - lo) / np.array(dims)))
    assert abs(cell * (depth > 0).sum() - 0.7183) < 0.02


def test_refusals_on_the_device_path(pt, ctx):
    refusals(pt, lambda *a, **k: _raw(pt, *a, host=False, ctx=ctx.handle, **k))
    pos, idx, dims, lo, hi = shapes(pt)["octahedron"]
    out = np.zeros(dims[::-1], np.float32)
    lo_a, hi_a = np.array(lo), np.array(hi)
    assert pt.lib.pt_mesh_sdf(None, None, len(pos), pos.ctypes.data, len(idx), idx.ctypes.data, *dims, lo_a.ctypes.data, hi_a.ctypes.data, out.ctypes.data) == -1
    assert "context" in pt.lib.pt_last_error().decode() and not out.any()


# ---- the result at work ---------------------------------------------------------------------------------------------------------------------
def test_density_feeds_the_grid_medium(pt, ctx, spot):
    pos, idx, dims, lo, hi = spot
    h = (hi[0] - lo[0]) / dims[0]
    grid = twin(pt, ctx, pos, idx, dims, lo, hi, what="density", ramp=2.0 * h)
    assert grid.min() == 0.0 and grid.max() == 1.0
    gs = pt.Scene(ctx)
    med = gs.mat_medium_grid(4.0, (0.9, 0.9, 0.9), 0.0, grid, lo, hi)
    assert med >= 0
    k, j, i = np.unravel_index(int(np.argmax(grid)), grid.shape)
    centre = lo + (np.array([i, j, k]) + 0.5) * (hi - lo) / np.array(dims)
    sigma = gs.medium_probe(med, 2, np.array([centre, lo - 1.0]))
    gs.close()
    assert abs(sigma[0] - 4.0) < 1e-9 and sigma[1] == 0.0                       # at a sample centre the trilinear value is the sample


def test_depth_feeds_isosurface(pt, ctx):
    pos, idx, dims, lo, hi = shapes(pt)["torus"]
    dims = (26, 14, 24)
    depth = twin(pt, ctx, pos, idx, dims, lo, hi, band=0.5)
    got = ctx.isosurface(depth, lo, hi, iso=0.0, closed=True, outside=-0.5)
    want = pt.isosurface_host(pt.mesh_sdf_host(pos, idx, dims, lo, hi, band=0.5), lo, hi, iso=0.0, closed=True, outside=-0.5)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert_closed_manifold(got[1])


def test_rays_meet_the_remeshed_sphere(pt, ctx):
    """The sphere of the CPU file (itself the mesh of a sphere field of radius 0.7) voxelised and meshed again: rays aimed at its centre c
    land within 2 D of the radii the input mesh spans, D one cell diagonal. The input's points lie between in_lo, the distance from c to
    the mesh (the independent distance function), and in_hi, its furthest vertex (|p - c| is convex along a triangle). A vertex of the
    new mesh lies on a lattice edge, at most D long, whose endpoints have depths of opposite sign, so the edge crosses the input surface
    and the vertex lies within D of it; a triangle lies in one lattice cube, so any of its points lies within D of a vertex, hence
    within 2 D of a point q of the input, and ||p - c| - |q - c|| <= 2 D. As test_iso_gpu.py::test_rays_meet_the_sphere does, the rays
    start outside and every one must hit."""
    pos, idx, _, lo, hi = shapes(pt)["sphere"]
    c, r = np.array((0.03, -0.02, 0.05)), 0.7
    in_lo = float(S.point_distance(c[None], pos, idx)[0])
    in_hi = float(np.linalg.norm(pos.astype(np.float64) - c, axis=1).max())
    assert 0.6 < in_lo <= in_hi < 0.75
    dims = (48, 52, 44)
    D = float(np.linalg.norm((np.array(hi) - np.array(lo)) / np.array(dims)))
    depth = twin(pt, ctx, pos, idx, dims, lo, hi, band=4.0 * D)
    rp, ri, rn = ctx.isosurface(depth, lo, hi, iso=0.0, closed=True, outside=-4.0 * D)
    assert_closed_manifold(ri)
    d = np.random.default_rng(11).normal(size=(2048, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    gs = pt.Scene(ctx)
    grey = gs.mat_diffuse(gs.tex_solid_rgb(0.5, 0.5, 0.5), -1)
    gs.world_add_object(gs.mesh(1.0, rp, ri, rn, None, grey))
    gs.world_build()
    start = r + 5.0
    rays = np.zeros((len(d), 7))
    rays[:, 0:3], rays[:, 3:6] = c + start * d, -d
    out = gs.intersect(rays)
    gs.close()
    radius = start - out[:, 1]
    lower, upper = in_lo - 2.0 * D, in_hi + 2.0 * D
    print(f"hits {int(out[:, 0].sum())} of {len(d)}; radius {radius.min():.6f} .. {radius.max():.6f} in [{lower:.6f}, {upper:.6f}]")
    assert np.all(out[:, 0] == 1.0)
    assert radius.min() >= lower and radius.max() <= upper


# ---- the command line: pt_render -s 6 --mesh-smoke / --remesh ---------------------------------------------------------------------------------
def _render(pt, tmp_path, name, *flags):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    png = tmp_path / (name + ".png")
    r = subprocess.run([exe, "-q", "-s", "6", "--width", "96", "--spp", "4", "--assets", pt.ASSET_DIR, *flags, "--out", str(png)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return pt.load_png_rgb8(str(png))


def test_cli_mesh_smoke(pt, tmp_path):
    plain = _render(pt, tmp_path, "plain")
    cloud = _render(pt, tmp_path, "cloud", "--mesh-smoke", "4")
    changed = (plain != cloud).any(axis=2)
    print(f"{int(changed.sum())} of {changed.size} pixels differ")
    assert changed.sum() > 0.02 * changed.size                                  # spot stands in view
    assert np.array_equal(_render(pt, tmp_path, "again", "--mesh-smoke", "4"), cloud)
    assert (_render(pt, tmp_path, "coarse", "--mesh-smoke", "4,32") != cloud).any()


def test_cli_remesh(pt, tmp_path):
    plain = _render(pt, tmp_path, "plain")
    grown = _render(pt, tmp_path, "grown", "--remesh", "0.02")
    assert (plain != grown).any()
    assert (_render(pt, tmp_path, "same_size", "--remesh", "0") != grown).any()


def test_cli_refusals(pt, tmp_path):
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_render")
    out = tmp_path / "bad.png"
    form, pair = "--mesh-smoke must be SCALE[,GRID_N[,RAMP_CELLS]]", "--mesh-smoke cannot be combined with"
    reform = "--remesh must be OFFSET[,GRID_N]"
    # (an unknown flag exits with 2 and names itself too: each case asks for the text of the new parser's own message)
    cases = ((("--mesh-smoke", "x"), form), (("--mesh-smoke", "0"), form), (("--mesh-smoke", "-1"), form), (("--mesh-smoke", "4,7"), form), (("--mesh-smoke", "4,257"), form),
             (("--mesh-smoke", "4,32.5"), form), (("--mesh-smoke", "4,32,0"), form), (("--mesh-smoke", "4,32,2,1"), form), (("--mesh-smoke", "4", "--smoke", "1"), pair),
             (("--mesh-smoke", "4", "--fog", "0.1"), pair), (("--mesh-smoke", "4", "--isosurface", "0.3"), pair), (("--mesh-smoke", "4", "--env-sampling", "0.5"), pair),
             (("--mesh-smoke", "4", "--subdivide", "1"), "--mesh-smoke and --subdivide cannot be combined"), (("--remesh", "0", "--subdivide", "1"), "--remesh and --subdivide cannot be combined"),
             (("--mesh-smoke", "4", "--remesh", "0"), "--mesh-smoke and --remesh cannot be combined"),
             (("--remesh", "x"), reform), (("--remesh", "0.02,7"), reform), (("--remesh", "0.02,257"), reform), (("--remesh", "0.02,64,1"), reform), (("--remesh", "nan"), reform),
             (("--remesh", "0.6"), reform))
    for flags, text in cases:
        r = subprocess.run([exe, "-q", "-s", "6", "--width", "32", "--spp", "1", "--assets", pt.ASSET_DIR, *flags, "--out", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and text in r.stderr, (flags, r.stderr)
        assert not out.exists()
    for flag, arg in (("--mesh-smoke", "4"), ("--remesh", "0.02")):                 # scene 6 only
        r = subprocess.run([exe, "-q", "-s", "3", "--width", "32", "--spp", "1", "--assets", pt.ASSET_DIR, flag, arg, "--out", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and flag + " works on scene 6 only" in r.stderr and not out.exists()
