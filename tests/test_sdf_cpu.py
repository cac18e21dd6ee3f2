"""Mesh voxelisation, the host twin (pt_mesh_sdf_host) against the header's rule restated in numpy (tests/sdf_rule.py): the
winding numbers and the occupancy exactly, the distance within ulp_f32(ref) + 1e-12 |box diagonal| of an independent formulation, and
against properties that need no rule: the closed form of an axis-aligned cube, ties on sample centres, inverted, nested and overlapping
bodies, degenerate triangles, boxes beside, inside and across the mesh, every mode, the band as a clip, spot's volume and the round trip
through isosurface extraction, pt_mesh_fit_grid's formula, every refusal. No GPU.

Spot: assets/spot.obj through mesh_fit_grid(pos, 26, 2.0), which gives 17 x 26 x 26 samples here (the issue's "about 16 x 24 x 26").
what = 3 against clip(depth / ramp, 0, 1) is an identity of bytes only where dividing by ramp commutes with the rounding to f32, so
that test uses a power of two for ramp."""
import ctypes as C
import os

import numpy as np
import pytest

import iso_rule as I
import sdf_rule as S
from test_iso_cpu import assert_closed_manifold

LO, HI = (-1.0, 0.5, 2.0), (3.5, 4.5, 5.5)               # a box that is not a cube


def _iso_mesh(pt, field, lo, hi):
    pos, idx, nrm = pt.isosurface_host(field, lo, hi, iso=0.0, closed=True, outside=-1.0, normals="none")
    return pos, idx


_CACHE = {}


def shapes(pt):
    """name -> (pos, idx, dims, lo, hi): shared with test_sdf_gpu.py; built once"""
    if _CACHE:
        return _CACHE
    out = _CACHE
    out["tetrahedron"] = (*S.tetrahedron(), (9, 6, 11), (-0.4, -0.3, -0.2), (1.9, 1.8, 1.6))
    out["octahedron"] = (*S.octahedron((1.2, 2.4, 3.7), 0.9), (11, 9, 6), LO, HI)
    out["cube"] = (*S.cube((0.1, 1.2, 2.6), (2.3, 3.9, 4.8)), (12, 10, 7), LO, HI)
    lo, hi = (-2.0, -1.0, -2.0), (2.0, 1.0, 2.0)
    out["torus"] = (*_iso_mesh(pt, I.torus_field((8, 5, 8), lo, hi, (0.05, 0.02, -0.03), 1.2, 0.45), lo, hi), (13, 7, 12), (-2.1, -1.1, -2.2), (2.2, 1.2, 2.1))
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    out["sphere"] = (*_iso_mesh(pt, I.sphere_field((6, 5, 6), lo, hi, (0.03, -0.02, 0.05), 0.7), lo, hi), (9, 10, 8), (-1.0, -1.1, -0.9), (1.1, 1.0, 1.0))
    return out


def host(pt, name_or_mesh, **kw):
    pos, idx, dims, lo, hi = name_or_mesh
    return pt.mesh_sdf_host(pos, idx, dims, lo, hi, **kw)


def same(got, want):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32))
        raise AssertionError(f"{len(bad)} of {got.size} values differ, first at {bad[0]}: {got.reshape(-1)[bad[0]]!r} vs {want.reshape(-1)[bad[0]]!r}")


def check_against_rule(pt, mesh, run=None):
    """depth, distance and occupancy of a mesh against the numpy rule -> (depth, winding)"""
    run = run or (lambda **kw: host(pt, mesh, **kw))
    pos, idx, dims, lo, hi = mesh
    ref, w = S.depth(pos, idx, dims, lo, hi)
    for fill in ("nonzero", "odd"):
        occ = run(what="occupancy", fill=fill)
        assert np.array_equal(occ, S.inside(w, fill).astype(np.float32))
    got = run(what="depth")
    tol = S.tolerance(ref, lo, hi)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"depth: max error {err.max():.3e}, largest error / tolerance {(err / tol).max():.3f}")
    assert np.all(err <= tol)
    assert np.array_equal(np.signbit(got), ~S.inside(w))
    same(run(what="distance"), np.abs(got))
    return got, w


@pytest.mark.parametrize("name", ("tetrahedron", "octahedron", "cube", "torus", "sphere"))
def test_shape_matches_rule(pt, name):
    mesh = shapes(pt)[name]
    got, w = check_against_rule(pt, mesh)
    assert set(np.unique(w)) == {0, 1}
    if name in ("torus", "sphere"):
        assert_closed_manifold(mesh[1])
        assert 200 < len(mesh[1]) // 3 < 1000


def test_default_options_are_the_wrappers(pt):
    o = pt.SdfOpts()
    d = pt.SdfOpts(what=3, fill=1, negate=True, band=2.0, ramp=5.0)
    assert pt.lib.pt_sdf_opts_default(C.byref(d)) == 0
    assert bytes(o) == bytes(d) and (d.what, d.fill, d.negate, d.band, d.ramp) == (0, 0, 0, 0.0, 0.0)
    assert pt.lib.pt_sdf_opts_default(None) == -1
    pos, idx, dims, lo, hi = shapes(pt)["cube"]
    out = np.zeros(dims[::-1], np.float32)
    lo_a, hi_a = np.array(lo), np.array(hi)
    assert pt.lib.pt_mesh_sdf_host(None, len(pos), pos.ctypes.data, len(idx), idx.ctypes.data, *dims, lo_a.ctypes.data, hi_a.ctypes.data, out.ctypes.data) == 0
    same(out, host(pt, shapes(pt)["cube"]))


def test_cube_closed_form(pt):
    pos, idx, dims, lo, hi = shapes(pt)["cube"]
    c0, c1 = pos.astype(np.float64).min(axis=0), pos.astype(np.float64).max(axis=0)
    p = S.grid_points(dims, lo, hi)
    q = np.maximum(np.maximum(c0 - p, p - c1), 0.0)
    outside = np.sqrt((q * q).sum(axis=1))
    within = np.minimum(p - c0, c1 - p).min(axis=1)
    ref = np.where(outside > 0, -outside, within).reshape(dims[::-1])
    got = host(pt, shapes(pt)["cube"])
    assert np.all(np.abs(got - ref) <= S.tolerance(ref, lo, hi))
    assert (got > 0).sum() > 20 and (got < 0).sum() > 20


def test_ties_cube_on_sample_centres(pt):
    """Faces, edges and vertices exactly on sample centres (dyadic coordinates): the body is the half-open [c0, c1)^3"""
    dims, lo, hi = (8, 8, 8), (0.0, 0.0, 0.0), (4.0, 4.0, 4.0)                 # centres at 0.25 + 0.5 i
    c0, c1 = (0.75, 1.25, 0.25), (2.75, 3.25, 2.25)
    mesh = (*S.cube(c0, c1), dims, lo, hi)
    p = S.grid_points(dims, lo, hi)
    want = np.all((p >= np.array(c0)) & (p < np.array(c1)), axis=1).reshape(8, 8, 8)
    occ = host(pt, mesh, what="occupancy")
    assert np.array_equal(occ, want.astype(np.float32))
    assert want.sum() == 4 * 4 * 4
    got, w = check_against_rule(pt, mesh)
    on_surface = got == 0
    assert on_surface.sum() == 5 ** 3 - 3 ** 3                                  # the samples on the cube's surface: d = 0, either sign
    assert np.array_equal(host(pt, mesh, what="occupancy"), (~np.signbit(got)).astype(np.float32))


def test_ties_octahedron_vertices_on_sample_centres(pt):
    dims, lo, hi = (8, 8, 8), (0.0, 0.0, 0.0), (4.0, 4.0, 4.0)
    mesh = (*S.octahedron((1.75, 2.25, 1.75), 1.5), dims, lo, hi)             # vertices, and the centre, on sample centres
    got, w = check_against_rule(pt, mesh)
    assert set(np.unique(w)) == {0, 1}
    # |x| + |y| + |z| < r strictly inside; on the surface the rule's tie decides, but no sample further out is inside
    p = S.grid_points(dims, lo, hi) - np.array((1.75, 2.25, 1.75))
    l1 = np.abs(p).sum(axis=1).reshape(8, 8, 8)
    assert np.all(w[l1 < 1.5] == 1) and np.all(w[l1 > 1.5] == 0)
    assert (l1 == 1.5).sum() > 6 and 0 < w[l1 == 1.5].sum() < (l1 == 1.5).sum()


def test_inside_out(pt):
    pos, idx, dims, lo, hi = shapes(pt)["cube"]
    mesh = (pos, S.flipped(idx), dims, lo, hi)
    w = S.winding(*mesh)
    assert set(np.unique(w)) == {-1, 0}
    want = host(pt, shapes(pt)["cube"])
    for fill in ("nonzero", "odd"):
        same(host(pt, mesh, fill=fill), want)


def test_shell(pt):
    dims, lo, hi = (10, 9, 8), (0.0, 0.0, 0.0), (5.0, 4.5, 4.0)
    outer, inner = S.cube((0.6, 0.6, 0.6), (4.4, 3.9, 3.4)), S.cube((1.6, 1.6, 1.6), (3.4, 2.9, 2.4))
    mesh = (*S.merged(outer, (inner[0], S.flipped(inner[1]))), dims, lo, hi)
    got, w = check_against_rule(pt, mesh)
    p = S.grid_points(dims, lo, hi)
    in_outer = np.all((p > 0.6) & (p < np.array((4.4, 3.9, 3.4))), axis=1)
    in_inner = np.all((p > 1.6) & (p < np.array((3.4, 2.9, 2.4))), axis=1)
    assert np.array_equal(w.reshape(-1), (in_outer & ~in_inner).astype(np.int32))
    assert in_inner.sum() > 0 and np.all(got.reshape(-1)[in_inner] < 0)


def test_overlap(pt):
    dims, lo, hi = (10, 9, 8), (0.0, 0.0, 0.0), (5.0, 4.5, 4.0)
    mesh = (*S.merged(S.cube((0.6, 0.6, 0.6), (3.1, 3.1, 3.1)), S.cube((1.9, 1.4, 0.9), (4.4, 3.9, 3.4))), dims, lo, hi)
    got, w = check_against_rule(pt, mesh)
    assert set(np.unique(w)) == {0, 1, 2}
    nonzero, odd = host(pt, mesh, what="occupancy"), host(pt, mesh, what="occupancy", fill="odd")
    assert np.all(nonzero[w == 2] == 1.0) and np.all(odd[w == 2] == 0.0)
    assert np.array_equal(nonzero[w != 2], odd[w != 2])


def test_degenerates_change_nothing(pt):
    pos, idx, dims, lo, hi = shapes(pt)["sphere"]
    extra_pos = np.concatenate([pos, np.array([[0.125, 0.25, 0.375], [0.25, 0.5, 0.75], [0.5, 1.0, 1.5]], np.float32)])   # three points in a line, exactly
    n = len(pos)
    junk = np.array([n, n + 1, n + 2, 5, 5, 9, 7, 3, 7, n + 1, n + 1, n + 1], np.uint32)                             # zero area; repeated indices
    mixed = np.concatenate([idx[:30], junk[:6], idx[30:], junk[6:]])
    for kw in (dict(), dict(what="distance"), dict(what="occupancy"), dict(what="density", ramp=0.3)):
        same(pt.mesh_sdf_host(extra_pos, mixed, dims, lo, hi, **kw), pt.mesh_sdf_host(pos, idx, dims, lo, hi, **kw))
    with pytest.raises(pt.PtError, match="no triangle is left"):
        pt.mesh_sdf_host(extra_pos, junk, dims, lo, hi)
    assert not pt.mesh_sdf_host(extra_pos, junk, dims, lo, hi, what="occupancy").any()   # no distance pass: nothing to refuse


@pytest.mark.parametrize("where", ("beside", "inside_the_mesh", "across"))
def test_box_placement(pt, where):
    pos, idx = S.octahedron((0.1, 0.2, 0.3), 2.0)
    lo, hi = {"beside": ((3.0, 2.5, 4.0), (4.5, 3.5, 5.5)),                    # the mesh wholly outside the box
              "inside_the_mesh": ((-0.2, 0.0, 0.1), (0.3, 0.4, 0.5)),          # a mesh far larger than the box
              "across": ((-0.5, -3.0, 0.2), (3.5, 1.0, 2.9))}[where]           # a box cutting the mesh
    got, w = check_against_rule(pt, (pos, idx, (7, 6, 5), lo, hi))
    if where == "beside":
        assert not w.any() and np.all(got < 0)
    elif where == "inside_the_mesh":
        assert w.all() and np.all(got > 0)
    else:
        assert 0 < w.sum() < w.size


def test_open_quad_distance(pt):
    pos = np.array([[0, 0, 0.5], [1, 0, 0.5], [1, 1, 0.5], [0, 1, 0.5]], np.float32)
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    dims, lo, hi = (6, 7, 5), (-0.5, -0.6, -0.2), (1.6, 1.5, 1.3)
    got = pt.mesh_sdf_host(pos, idx, dims, lo, hi, what="distance")
    p = S.grid_points(dims, lo, hi)
    q = np.stack([np.clip(p[:, 0], 0, 1), np.clip(p[:, 1], 0, 1), np.full(len(p), 0.5)], axis=1)
    ref = np.linalg.norm(p - q, axis=1).reshape(dims[::-1])
    assert np.all(np.abs(got - ref) <= S.tolerance(ref, lo, hi))
    assert np.all(np.abs(got - S.distance(pos, idx, dims, lo, hi)) <= S.tolerance(ref, lo, hi))


@pytest.mark.parametrize("name", ("cube", "torus"))
def test_modes(pt, name):
    mesh = shapes(pt)[name]
    depth = host(pt, mesh)
    same(host(pt, mesh, negate=True), -depth)
    same(host(pt, mesh, what="occupancy"), (~np.signbit(depth)).astype(np.float32))   # depth > 0, or depth >= 0 where d = 0 lies inside
    same(host(pt, mesh, what="distance"), np.abs(depth))
    same(host(pt, mesh, what="distance", negate=True), np.abs(depth))                 # negate is what = 0's
    ramp = 0.25                                                                       # a power of two: / ramp commutes with the rounding to f32
    same(host(pt, mesh, what="density", ramp=ramp), np.clip(depth / np.float32(ramp), np.float32(0), np.float32(1)) + np.float32(0))
    same(host(pt, mesh, what="density", ramp=ramp, band=0.01), host(pt, mesh, what="density", ramp=ramp))   # band is not what = 3's
    third = host(pt, mesh, what="density", ramp=1.0 / 3.0)
    inside = ~np.signbit(depth)
    assert np.all(third[~inside] == 0) and np.all(np.abs(third - np.clip(depth.astype(np.float64) * 3.0, 0, 1)) <= 3e-7)


@pytest.mark.parametrize("name", ("octahedron", "torus"))
def test_band_is_a_clip(pt, name):
    mesh = shapes(pt)[name]
    depth = host(pt, mesh)
    for band in (0.05, 0.3, 1.0 / 3.0, 100.0):
        b = np.float32(band)
        same(host(pt, mesh, band=band), np.clip(depth, -b, b))
        same(host(pt, mesh, band=band, what="distance"), np.minimum(np.abs(depth), b))
    assert np.abs(depth).max() > 0.3 > np.abs(depth).min()


# ---- spot ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spot(pt):
    pos, idx, uv = pt.load_obj(os.path.join(pt.ASSET_DIR, "spot.obj"))
    dims, lo, hi = pt.mesh_fit_grid(pos, 26, 2.0)
    band = 4.0 * (hi[0] - lo[0]) / dims[0]
    return pos, idx, dims, lo, hi, band, pt.mesh_sdf_host(pos, idx, dims, lo, hi, band=band)


def test_spot_winding_and_volume(pt, spot):
    pos, idx, dims, lo, hi, band, depth = spot
    print(f"spot: dims {dims}, box {lo} .. {hi}")
    assert dims[2] == 26 and 14 <= dims[0] <= 26 and 20 <= dims[1] <= 26
    w = S.winding(pos, idx, dims, lo, hi)
    assert set(np.unique(w)) == {0, 1}
    assert np.array_equal(pt.mesh_sdf_host(pos, idx, dims, lo, hi, what="occupancy"), (w != 0).astype(np.float32))
    assert np.array_equal(~np.signbit(depth), w != 0)
    h = (hi - lo) / np.array(dims)
    cell, r = float(h.prod()), 0.5 * float(np.linalg.norm(h))                   # r: half a cell diagonal, less than the band
    volume = S.signed_volume(pos, idx)
    lower, upper = cell * (depth > r).sum(), cell * (depth > -r).sum()
    print(f"spot: {lower:.4f} <= {volume:.4f} <= {upper:.4f}")
    assert abs(volume - 0.7183) < 1e-3
    assert lower <= volume <= upper                                             # a cell whose centre is deeper than r lies wholly inside


def test_spot_distance_sample(pt, spot):
    pos, idx, dims, lo, hi, band, depth = spot
    pts = S.grid_points(dims, lo, hi)
    pick = np.random.default_rng(3).choice(len(pts), 300, replace=False)
    ref = np.minimum(S.point_distance(pts[pick], pos, idx), band)
    got = np.abs(depth.reshape(-1)[pick])
    assert np.all(np.abs(got - ref) <= S.tolerance(ref, lo, hi))


def test_spot_round_trip(pt, spot):
    pos, idx, dims, lo, hi, band, depth = spot
    rp, ri, rn = pt.isosurface_host(depth, lo, hi, iso=0.0, closed=True, outside=-band)
    assert_closed_manifold(ri)
    assert len(ri) // 3 > 1000
    # the distance is 1-Lipschitz and an edge's endpoints bracket zero: a vertex lies within one cell diagonal of the surface
    diag = float(np.linalg.norm((hi - lo) / np.array(dims)))
    far = S.point_distance_within(rp.astype(np.float64), pos, idx, diag)                # (exact where it is at most diag, larger elsewhere)
    print(f"round trip: {len(rp)} vertices, furthest {far.max():.5f} of a bound {diag:.5f}")
    assert far.max() <= diag


# ---- pt_mesh_fit_grid -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_longest, margin", ((26, 2.0), (8, 0.0), (64, 2.0), (33, 1.5), (10, 4.25)))
def test_fit_grid_formula(pt, n_longest, margin):
    pos = np.array([[0.1, -2.0, 3.0], [1.7, 0.5, 3.25], [0.9, 1.1, 3.5], [1.0, -1.0, 3.1]], np.float32)
    dims, lo, hi = pt.mesh_fit_grid(pos, n_longest, margin)
    p = pos.astype(np.float64)
    blo, bhi = p.min(axis=0), p.max(axis=0)
    ext = bhi - blo
    h = ext.max() / (np.float64(n_longest) - 2.0 * margin)
    n = np.maximum(2.0, np.ceil(ext / h + 2.0 * margin))
    c, half = blo + 0.5 * ext, 0.5 * (n * h)
    assert dims == tuple(int(v) for v in n)
    assert np.array_equal(lo, c - half) and np.array_equal(hi, c + half)
    assert n_longest <= max(dims) <= n_longest + 1
    assert np.allclose((hi - lo) / np.array(dims), h, rtol=1e-14)              # cubic cells
    assert np.all(lo <= blo - (margin - 1.0) * h) and np.all(hi >= bhi + (margin - 1.0) * h)


def test_fit_grid_refusals(pt):
    pos = np.array([[0, 0, 0], [1, 2, 3]], np.float32)
    for n, m in ((5, 2.0), (4, 2.0), (1, 0.0), (0, 0.0), (8, -1.0), (8, np.nan), (8, np.inf)):
        with pytest.raises(pt.PtError):
            pt.mesh_fit_grid(pos, n, m)
    with pytest.raises(pt.PtError, match="no extent"):
        pt.mesh_fit_grid(pos[:1], 8, 2.0)
    with pytest.raises(pt.PtError, match="finite"):
        pt.mesh_fit_grid(np.array([[0, 0, np.inf], [1, 1, 1]], np.float32), 8, 2.0)
    with pytest.raises(pt.PtError, match="2\\^28"):
        pt.mesh_fit_grid(np.array([[0, 0, 0], [1, 1, 1]], np.float32), 1024, 2.0)
    d, lo, hi = np.zeros(3, np.uint32), np.zeros(3), np.zeros(3)
    for null in range(4):
        a = [pos.ctypes.data, d.ctypes.data, lo.ctypes.data, hi.ctypes.data]
        a[null] = None
        assert pt.lib.pt_mesh_fit_grid(2, a[0], 8, 2.0, a[1], a[2], a[3]) == -1


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _raw(pt, pos, idx, dims, lo, hi, host=True, ctx=None, null=(), n_pos=None, n_idx=None, opts="given", **kw):
    """The C entry point itself -> rc; the output must be untouched when it refuses. null: names among pos idx lo hi out passed as NULL"""
    pos, idx = np.ascontiguousarray(pos, np.float32).reshape(-1, 3), np.ascontiguousarray(idx, np.uint32)
    lo_a, hi_a = np.array(lo, np.float64), np.array(hi, np.float64)
    big = dims[0] * dims[1] * dims[2] > 1 << 20
    out = np.full(8 if big else dims[0] * dims[1] * dims[2] + 8, 7.0, np.float32)
    o = None if opts is None else pt.SdfOpts(**kw)
    ptr = lambda name, a: None if name in null else a.ctypes.data
    args = (None if o is None else C.byref(o), len(pos) if n_pos is None else n_pos, ptr("pos", pos), len(idx) if n_idx is None else n_idx, ptr("idx", idx), *dims,
            ptr("lo", lo_a), ptr("hi", hi_a), ptr("out", out))
    rc = pt.lib.pt_mesh_sdf_host(*args) if host else pt.lib.pt_mesh_sdf(ctx, *args)
    if rc != 0:
        assert rc == -1 and np.all(out == 7.0), "a refused call wrote something"
    else:
        assert np.all(out[-8:] == 7.0) and not np.all(out[:-8] == 7.0)
    return rc


def refusals(pt, raw):
    """Every refusal of the rule; raw(pos, idx, dims, lo, hi, **kw) -> rc"""
    pos, idx, dims, lo, hi = shapes(pt)["octahedron"]
    err = lambda: pt.lib.pt_last_error().decode()
    assert raw(pos, idx, dims, lo, hi) == 0
    assert raw(pos, idx, dims, lo, hi, opts=None) == 0
    for name in ("pos", "idx", "lo", "hi", "out"):
        assert raw(pos, idx, dims, lo, hi, null=(name,)) == -1 and "null" in err(), name
    for n_idx in (0, 1, 2, 4, 23):
        assert raw(pos, idx, dims, lo, hi, n_idx=n_idx) == -1 and "multiple of 3" in err()
    assert raw(pos, idx, dims, lo, hi, n_idx=3 * 0x08000000) == -1 and "0x07FFFFFF" in err()   # refused before an index is read
    for at, bad in ((0, 6), (23, 6), (5, 0xFFFFFFFF)):
        w = idx.copy()
        w[at] = bad
        assert raw(pos, w, dims, lo, hi) == -1 and "index" in err()
    assert raw(pos, idx, dims, lo, hi, n_pos=5) == -1 and "index" in err()
    for bad in (np.nan, np.inf, -np.inf):
        w = pos.copy()
        w[3, 1] = bad
        assert raw(w, idx, dims, lo, hi) == -1 and "position" in err()
        for a in range(3):
            l, h = list(lo), list(hi)
            l[a] = bad
            assert raw(pos, idx, dims, l, hi) == -1 and "box" in err()
            h[a] = bad
            assert raw(pos, idx, dims, lo, h) == -1 and "box" in err()
        assert raw(pos, idx, dims, lo, hi, band=bad) == -1 and "band" in err()
        assert raw(pos, idx, dims, lo, hi, what=3, ramp=bad) == -1 and "ramp" in err()
    for a in range(3):
        h = list(hi)
        h[a] = lo[a]
        assert raw(pos, idx, dims, lo, h) == -1 and "lo < hi" in err()
        h[a] = lo[a] - 1.0
        assert raw(pos, idx, dims, lo, h) == -1 and "lo < hi" in err()
    for n in ((1, 5, 5), (5, 1, 5), (5, 5, 1), (0, 2, 2)):
        assert raw(pos, idx, n, lo, hi) == -1 and "at least 2" in err()
    for n in ((1 << 14, 1 << 14, 2), (1 << 16, 1 << 16, 1 << 16), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), ((1 << 28) + 1, 2, 2)):
        assert raw(pos, idx, n, lo, hi) == -1 and "2^28" in err(), n
    for what in (-1, 4):
        assert raw(pos, idx, dims, lo, hi, what=what) == -1 and "what" in err()
    for fill in (-1, 2):
        assert raw(pos, idx, dims, lo, hi, fill=fill) == -1 and "fill" in err()
    assert raw(pos, idx, dims, lo, hi, band=-0.5) == -1 and "band" in err()
    for ramp in (0.0, -1.0, None):
        assert raw(pos, idx, dims, lo, hi, what=3, ramp=ramp) == -1 and "ramp" in err()
    assert raw(pos, idx, dims, lo, hi, what=0, ramp=-1.0) == 0                                 # the ramp is what = 3's alone
    flat = np.array([0, 0, 1, 2, 3, 3], np.uint32)
    assert raw(pos, flat, dims, lo, hi) == -1 and "no triangle is left" in err()


def test_refusals(pt):
    refusals(pt, lambda *a, **k: _raw(pt, *a, **k))
    pos, idx, dims, lo, hi = shapes(pt)["octahedron"]
    with pytest.raises(pt.PtError):
        pt.mesh_sdf_host(pos, idx, (1, 4, 4), lo, hi)
    with pytest.raises(pt.PtError):
        pt.mesh_sdf_host(pos, idx, (1 << 12, 1 << 12, 1 << 12), lo, hi)
    with pytest.raises(pt.PtError):
        pt.mesh_sdf_host(pos, idx, dims, lo, hi, what="density")                               # no ramp given
