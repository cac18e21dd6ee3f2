"""Isosurface extraction, the host twin (pt_mesh_isosurface_host) against the header's rule restated in numpy
(tests/iso_rule.py), byte for byte, and against properties that need no rule: closed, manifold and consistently wound meshes for all 256
corner patterns, the winding of every tetrahedron's triangles, the Euler characteristic, volume, radius bound and normals of a sphere, a
torus, ties, empty grids, chaining into Loop subdivision, every refusal. No GPU.

The sphere of the issue (9 x 8 x 7 samples, r > 4L) is larger than its grid, so the added layer of `outside` samples caps it where it
leaves the hull of the sample centres. A cap vertex lies on an edge to an added sample, whose value is `outside` and not the field's, so
the radius bound (which rests on the field along the edge) says nothing about it: the radius and direction checks run over the vertices
inside the hull, which are exactly those on edges between two samples; Euler characteristic, volume and unit normals over the whole mesh.
sphere_whole (24 x 22 x 20, the same r > 4L) lies inside its grid, and there every vertex is held to the bound."""
import ctypes as C

import numpy as np
import pytest

import iso_rule as I

LO, HI = (-1.0, 0.5, 2.0), (3.5, 4.5, 5.5)               # a box that is not a cube


def _sphere(n, lo, hi, centre=None, r_over_L=4.05):
    h = (np.array(hi) - np.array(lo)) / np.array(n, dtype=np.float64)
    L = float(np.sqrt((h * h).sum()))                   # the longest lattice edge: the cube diagonal
    r = r_over_L * L
    mid = 0.5 * (np.array(lo) + np.array(hi)) + 0.3 * h
    # a sphere of r > 4L that lay about the middle of 9 x 8 x 7 samples would swallow them all: its centre is moved out along a skew
    # direction until the surface passes through the middle of the grid. The larger grid holds the whole sphere.
    out = r * np.array([0.6, -0.64, 0.48]) if min(n) < 16 else 0.0
    c = mid + out if centre is None else np.array(centre)
    return I.sphere_field(n, lo, hi, c, r), c, r, L, h


def _shapes():
    """name -> (values [k, j, i], lo, hi, kwargs): shared with test_iso_gpu.py"""
    out = {}
    v, c, r, L, h = _sphere((9, 8, 7), LO, HI)
    out["sphere"] = (v, LO, HI, dict(iso=0.0, closed=True, outside=-1.0))
    out["sphere_open"] = (v, LO, HI, dict(iso=0.0, closed=False))
    v, c, r, L, h = _sphere((24, 22, 20), LO, HI)
    out["sphere_whole"] = (v, LO, HI, dict(iso=0.0, closed=True, outside=-1.0))
    lo, hi = (-2.0, -1.0, -2.0), (2.0, 1.0, 2.0)
    out["torus"] = (I.torus_field((22, 12, 20), lo, hi, (0.05, 0.02, -0.03), 1.2, 0.45), lo, hi, dict(iso=0.0, closed=True, outside=-1.0))
    k, j, i = np.meshgrid(np.arange(4), np.arange(5), np.arange(6), indexing="ij")
    ties = ((i + 2 * j + 3 * k) % 3).astype(np.float32)                    # 0, 1, 2: a third of the samples equal iso = 1
    out["ties"] = (ties, LO, HI, dict(iso=1.0, closed=False))
    out["ties_closed"] = (ties, LO, HI, dict(iso=1.0, closed=True, outside=1.0))   # `outside` itself equal to iso: inside
    rng = np.random.default_rng(29)
    out["noise_negative"] = ((rng.random((5, 6, 7)) * 4.0 - 5.0).astype(np.float32), LO, HI, dict(iso=-2.75, closed=True, outside=-7.0))
    out["plume_like"] = ((rng.random((6, 5, 9)) ** 3).astype(np.float32), LO, HI, dict(iso=0.3))
    return out


SHAPES = _shapes()
NORMALS = ("gradient", "smooth", "none")


def same(got, want):
    assert len(got) == len(want) == 3
    for name, g, w in zip(("pos", "idx", "nrm"), got, want):
        if w is None:
            assert g is None, f"{name}: expected none"
            continue
        assert g is not None, f"{name}: missing"
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.reshape(-1).view(np.uint32) != w.reshape(-1).view(np.uint32))
            raise AssertionError(f"{name}: {len(bad)} of {g.size} values differ, first at {bad[0]}: {g.reshape(-1)[bad[0]]!r} vs {w.reshape(-1)[bad[0]]!r}")


def pattern(bits, iso):
    """The 2 x 2 x 2 grid whose corner c = x + 2y + 4z is inside when bit c is set: values iso +- 1"""
    v = np.array([iso + 1.0 if bits >> c & 1 else iso - 1.0 for c in range(8)], dtype=np.float32)
    return v.reshape(2, 2, 2)


def edge_use(idx):
    """{directed edge (a, b): how many triangles run along it}"""
    tri = np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    use = {}
    for a, b in np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]):
        use[(int(a), int(b))] = use.get((int(a), int(b)), 0) + 1
    return use


def assert_closed_manifold(idx):
    use = edge_use(idx)
    for (a, b), n in use.items():
        assert a != b
        assert n == 1 and use.get((b, a), 0) == 1, f"edge ({a}, {b}): {n} times, reversed {use.get((b, a), 0)} times"


def euler(pos, idx):
    use = edge_use(idx)
    E = len({(min(a, b), max(a, b)) for a, b in use})
    return len(pos) - E + len(idx) // 3


def signed_volume(pos, idx):
    p = pos.astype(np.float64)[np.asarray(idx, dtype=np.int64).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ---- the twin against the rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normals", NORMALS)
@pytest.mark.parametrize("closed", (False, True))
def test_all_corner_patterns(pt, closed, normals):
    iso = 0.25
    for bits in range(256):
        v = pattern(bits, iso)
        kw = dict(iso=iso, closed=closed, outside=iso - 1.0, normals=normals)
        got = pt.isosurface_host(v, LO, HI, **kw)
        same(got, I.isosurface(v, LO, HI, **kw))
        use = edge_use(got[1])
        if closed:
            assert_closed_manifold(got[1])
            assert (len(got[1]) == 0) == (bits == 0)
        else:
            assert all(n + use.get((b, a), 0) <= 2 for (a, b), n in use.items())
            assert all(n == 1 for n in use.values())                     # and never twice in the same direction
        if got[2] is not None and normals == "gradient":
            assert np.all(np.abs(np.linalg.norm(got[2].astype(np.float64), axis=1) - 1.0) < 1e-6)


@pytest.mark.parametrize("normals", NORMALS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_matches_rule(pt, name, normals):
    v, lo, hi, kw = SHAPES[name]
    same(pt.isosurface_host(v, lo, hi, normals=normals, **kw), I.isosurface(v, lo, hi, normals=normals, **kw))


def test_default_options_are_the_wrappers(pt):
    o = pt.IsoOpts(1.0, 1, 2.0, 2)
    assert pt.lib.pt_iso_opts_default(C.byref(o)) == 0
    assert (o.iso, o.closed, o.outside, o.normals) == (0.5, 0, 0.0, 0)
    d = pt.IsoOpts()
    assert (d.iso, d.closed, d.outside, d.normals) == (0.5, 0, 0.0, 0)
    v = SHAPES["plume_like"][0]
    assert _raw(pt, v, LO, HI, opts=None)[0] == 0                          # NULL options: the defaults
    same(_raw(pt, v, LO, HI, opts=None)[1], pt.isosurface_host(v, LO, HI))


# ---- the case table, through the winding property -------------------------------------------------------------------------------------------
def test_winding_of_every_tetrahedron(pt):
    """One cube, open, values iso +- 1, so every vertex is an edge's midpoint. The triangles come in (tetrahedron, triangle) order and a
    tetrahedron with 1 / 2 / 3 corners inside gives 1 / 2 / 1 of them: that assigns each triangle its tetrahedron without the table."""
    lo, h = np.array(LO), (np.array(HI) - np.array(LO)) / 2.0
    seen = 0
    for bits in range(256):
        pos, idx, _ = pt.isosurface_host(pattern(bits, 0.0), LO, HI, iso=0.0, normals="none")
        lat = np.round(((pos.astype(np.float64) - lo) / h - 0.5) * 2.0) / 2.0      # lattice coordinates: multiples of one half
        tri = idx.reshape(-1, 3)
        f = 0
        for tet in I.TETS:
            corners = np.array([I.corner_xyz(c) for c in tet], dtype=np.float64)
            ins = np.array([bool(bits >> c & 1) for c in tet])
            count = (0, 1, 2, 1, 0)[int(ins.sum())]
            mids = {tuple(0.5 * (corners[a] + corners[b])) for a in range(4) for b in range(4) if ins[a] and not ins[b]}
            used = set()
            for t in tri[f:f + count]:
                p = lat[t]
                assert all(tuple(q) in mids for q in p), (bits, tet)
                used.update(tuple(q) for q in p)
                want = corners[~ins].mean(axis=0) - corners[ins].mean(axis=0)
                assert np.dot(np.cross(p[1] - p[0], p[2] - p[0]), want) > 0, (bits, tet)
                seen += 1
            assert used == mids                                                       # every crossing edge of the tetrahedron is used
            f += count
        assert f == len(tri)
    assert seen == 6 * 16 * 20              # each tetrahedron meets each of its 16 cases 16 times; the cases hold 20 triangles


# ---- the sphere ---------------------------------------------------------------------------------------------------------------------------
def _radius_bound(r, L):
    return r - L * L / (4.0 * (r - 2.0 * L)), r * (1.0 + 1e-6)


@pytest.mark.parametrize("who", ("rule", "twin"))
@pytest.mark.parametrize("n", ((9, 8, 7), (24, 22, 20)))
def test_sphere(pt, n, who):
    v, c, r, L, h = _sphere(n, LO, HI)
    assert r > 4.0 * L
    kw = dict(iso=0.0, closed=True, outside=-1.0)
    pos, idx, nrm = I.isosurface(v, LO, HI, **kw) if who == "rule" else pt.isosurface_host(v, LO, HI, **kw)
    assert_closed_manifold(idx)
    assert euler(pos, idx) == 2
    assert signed_volume(pos, idx) > 0.0
    hull_lo, hull_hi = (np.array(LO) + 0.5 * h).astype(np.float32), (np.array(HI) - 0.5 * h).astype(np.float32)
    field = np.all((pos >= hull_lo) & (pos <= hull_hi), axis=1)            # on an edge between two samples (see the module's docstring)
    whole = n == (24, 22, 20)
    assert field.all() == whole and field.sum() > 100
    d = pos.astype(np.float64) - c
    rad = np.linalg.norm(d, axis=1)
    lower, upper = _radius_bound(r, L)
    print(f"{who} {n}: {len(pos)} vertices, {int(field.sum())} on field edges; radius {rad[field].min():.6f} .. {rad[field].max():.6f} in [{lower:.6f}, {upper:.6f}], r {r:.6f}")
    assert rad[field].min() >= lower and rad[field].max() <= upper
    N = nrm.astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(N, axis=1) - 1.0) < 1e-6)
    assert np.all(np.einsum("ij,ij->i", N[field], d[field]) > 0.0)


def test_torus(pt):
    v, lo, hi, kw = SHAPES["torus"]
    pos, idx, nrm = pt.isosurface_host(v, lo, hi, **kw)
    assert_closed_manifold(idx)
    assert euler(pos, idx) == 0
    assert signed_volume(pos, idx) > 0.0
    assert np.all(np.abs(pos) < np.array(hi, dtype=np.float32) - 0.1)      # it lies inside its grid: no cap


def test_ties(pt):
    """Samples equal to iso are inside, t = 0 puts their edges' vertices on the sample itself: coincident vertices and zero-area
    triangles are kept, and the connectivity is still closed."""
    v, lo, hi, kw = SHAPES["ties_closed"]
    pos, idx, nrm = pt.isosurface_host(v, lo, hi, **kw)
    assert_closed_manifold(idx)
    assert len(np.unique(pos, axis=0)) < len(pos)
    p = pos.astype(np.float64)[idx.reshape(-1, 3).astype(np.int64)]
    area = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    assert (area == 0.0).any() and (area > 0.0).any()
    assert np.isfinite(nrm).all() and np.all(np.abs(nrm).max(axis=1) > 0)


def test_empty(pt):
    ones = np.ones((3, 4, 5), np.float32)
    for v, kw in ((ones, dict(iso=0.5)), (ones, dict(iso=1.0)), (ones, dict(iso=1.5)), (ones, dict(iso=1.5, closed=True, outside=0.0)), (-ones, dict(iso=-0.5))):
        for normals in NORMALS:
            pos, idx, nrm = pt.isosurface_host(v, LO, HI, normals=normals, **kw)
            assert pos.shape == (0, 3) and idx.shape == (0,) and (nrm is None) == (normals == "none")
            same((pos, idx, nrm), I.isosurface(v, LO, HI, normals=normals, **kw))
    pos, idx, _ = pt.isosurface_host(ones, LO, HI, iso=0.5, closed=True)    # all inside and closed: the box of the sample centres' hull, grown
    assert_closed_manifold(idx)
    assert euler(pos, idx) == 2


def test_chaining_into_subdivision(pt):
    v, lo, hi, kw = SHAPES["sphere"]
    pos, idx, nrm = pt.isosurface_host(v, lo, hi, **kw)
    p, i, n, uv, crease = pt.subdivide_host(pos, idx)
    E = len({(min(a, b), max(a, b)) for a, b in edge_use(idx)})
    assert len(p) == len(pos) + E and len(i) == 4 * len(idx)
    assert not crease.any()
    assert_closed_manifold(i)                                               # no boundary edge went in, none comes out
    assert euler(p, i) == 2
    # a boundary edge would have been sharp: its midpoint exactly (A + B) / 2. With none, no odd vertex of a curved patch sits there
    q, j, _, _, _ = pt.subdivide_host(pos, idx, crease=np.ones(len(idx), np.uint8))
    assert np.array_equal(i, j) and (p[len(pos):] != q[len(pos):]).any(axis=1).mean() > 0.9


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _raw(pt, values, lo, hi, opts="default", host=True, ctx=None, null=(), n=None, **kw):
    """The C entry point itself -> (rc, mesh or None). null: names among pos n_pos idx n_idx nrm values lo hi passed as NULL"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    nz, ny, nx = values.shape if n is None else n[::-1]
    lo_a, hi_a = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    o = None if opts is None else pt.IsoOpts(**kw)
    pos, idx, nrm = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)()
    n_pos, n_idx = C.c_uint32(), C.c_uint32()
    ref = lambda name, x: None if name in null else C.byref(x)
    args = (None if o is None else C.byref(o), nx, ny, nz, None if "values" in null else values.ctypes.data, None if "lo" in null else lo_a.ctypes.data,
            None if "hi" in null else hi_a.ctypes.data, ref("pos", pos), ref("n_pos", n_pos), ref("idx", idx), ref("n_idx", n_idx), ref("nrm", nrm))
    rc = pt.lib.pt_mesh_isosurface_host(*args) if host else pt.lib.pt_mesh_isosurface(ctx, *args)
    if rc != 0:
        assert not pos and not idx and not nrm, "a refused call left an output behind"
        return rc, None
    nv, ni = n_pos.value, n_idx.value
    mesh = (np.ctypeslib.as_array(pos, (nv * 3,)).copy().reshape(-1, 3) if nv else np.zeros((0, 3), np.float32),
            np.ctypeslib.as_array(idx, (ni,)).copy() if ni else np.zeros(0, np.uint32),
            (np.ctypeslib.as_array(nrm, (nv * 3,)).copy().reshape(-1, 3) if nv else np.zeros((0, 3), np.float32)) if nrm else None)
    for p in (pos, idx, nrm):
        if p:
            pt.lib.pt_free(p)
    return rc, mesh


def refusals(pt, raw):
    """Every refusal of the rule; raw(values, lo, hi, **kw) -> (rc, mesh)"""
    v = SHAPES["plume_like"][0]
    assert raw(v, LO, HI)[0] == 0
    for name in ("pos", "n_pos", "idx", "n_idx", "nrm", "values", "lo", "hi"):
        assert raw(v, LO, HI, null=(name,))[0] == -1, name
        assert {"values": "values", "lo": "box", "hi": "box"}.get(name, "output") in pt.lib.pt_last_error().decode()
    for n in ((1, 5, 5), (5, 1, 5), (5, 5, 1), (0, 2, 2)):
        assert raw(v, LO, HI, n=n)[0] == -1 and "at least 2" in pt.lib.pt_last_error().decode()
    # sizes are refused before a value is read: the array need not be that large
    for n in ((1 << 14, 1 << 14, 2), (1 << 16, 1 << 16, 1 << 16), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), ((1 << 28) + 1, 2, 2)):
        assert raw(v, LO, HI, n=n)[0] == -1 and "2^28" in pt.lib.pt_last_error().decode(), n
    assert raw(v, LO, HI, n=(1 << 26, 2, 2), closed=1)[0] == -1 and "2^29" in pt.lib.pt_last_error().decode()     # 2^28 samples, (2^26 + 2) 16 lattice points
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[-1, -1, -1] = bad
        assert raw(w, LO, HI)[0] == -1 and "value" in pt.lib.pt_last_error().decode()
        assert raw(v, LO, HI, iso=bad)[0] == -1 and "iso" in pt.lib.pt_last_error().decode()
        assert raw(v, LO, HI, outside=bad)[0] == -1 and "outside" in pt.lib.pt_last_error().decode()
        assert raw(v, LO, HI, outside=bad, closed=1)[0] == -1
        for a in range(3):
            lo, hi = list(LO), list(HI)
            lo[a] = bad
            assert raw(v, lo, HI)[0] == -1 and "box" in pt.lib.pt_last_error().decode()
            hi[a] = bad
            assert raw(v, LO, hi)[0] == -1 and "box" in pt.lib.pt_last_error().decode()
    for a in range(3):
        hi = list(HI)
        hi[a] = LO[a]
        assert raw(v, LO, hi)[0] == -1 and "lo < hi" in pt.lib.pt_last_error().decode()
        hi[a] = LO[a] - 1.0
        assert raw(v, LO, hi)[0] == -1 and "lo < hi" in pt.lib.pt_last_error().decode()
    for closed in (-1, 2):
        assert raw(v, LO, HI, closed=closed)[0] == -1 and "closed" in pt.lib.pt_last_error().decode()
    for normals in (-1, 3):
        assert raw(v, LO, HI, normals=normals)[0] == -1 and "normals" in pt.lib.pt_last_error().decode()


def test_refusals(pt):
    refusals(pt, lambda *a, **k: _raw(pt, *a, **k))
    with pytest.raises(pt.PtError):
        pt.isosurface_host(np.ones((1, 2, 2), np.float32), LO, HI)
    with pytest.raises(ValueError):
        pt.isosurface_host(np.ones((2, 2), np.float32), LO, HI)
