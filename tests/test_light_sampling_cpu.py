"""Exact light sampling without a GPU: the ABI's new symbols, and the rule itself (tests/light_rule.py, a numpy restatement of
include/pt_amd.h) — the mesh sampler is uniform by area, its pdf integrates to 1, and the fixed-seed ray sets of the GPU probe test
leave almost nothing out."""
import ctypes
import os

import numpy as np

import light_rule as LR
from common import icosphere

NEW_SYMBOLS = ("pt_scene_set_light_sampling", "pt_scene_light_sampling", "pt_light_probe")


def test_library_exports_the_new_symbols(pt):
    lib = ctypes.CDLL(pt.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pt_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pt.ABI_SYMBOLS and name + "(" in header
    assert pt.LIGHT_SAMPLING == {"reference": 0, "exact": 1}


def test_mesh_sampler_is_uniform_by_area():
    """Chi-square over the faces of the 128-triangle irregular mesh (areas differ by more than 10x). 127 degrees of freedom: the
    0.9999 quantile of chi2_127 is 195 (Wilson-Hilferty), so a correct sampler fails once in 10^4 seeds — and this seed is fixed.
    The reference's choice, a uniform face, misses by orders of magnitude."""
    P, I = LR.tessellate_quad((-1.0, 0.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), 8)
    tris = LR.mesh_tris(P, I)
    C = LR.area_table(tris)
    areas = np.diff(C)
    assert len(tris) == 128 and areas.max() > 10.0 * areas.min() and abs(C[-1] - 4.0) < 1e-6
    n = 200000
    rng = np.random.default_rng(5)
    u0, u1, u2 = rng.random(n), rng.random(n), rng.random(n)
    face, _, pts = LR.sample_mesh(C, tris, np.tile([0.3, 2.0, -0.2], (n, 1)), u0, u1, u2)
    expect = n * areas / C[-1]
    assert expect.min() > 20.0
    chi2 = float((((np.bincount(face, minlength=128) - expect) ** 2) / expect).sum())
    uniform = float((((np.bincount(rng.integers(0, 128, n), minlength=128) - expect) ** 2) / expect).sum())
    print(f"chi2 over 128 faces, {n} samples: area-weighted {chi2:.1f}, a uniform face choice {uniform:.0f}")
    assert chi2 < 195.0 and uniform > 100.0 * 195.0
    # the points are uniform over the quad as well: the 4 x 4 equal cells of [-1, 1]^2 (15 degrees of freedom, 0.9999 quantile 44.3)
    cell = np.minimum(((pts[:, 0] + 1.0) * 2.0).astype(int), 3) * 4 + np.minimum(((pts[:, 2] + 1.0) * 2.0).astype(int), 3)
    chi2_xy = float((((np.bincount(cell, minlength=16) - n / 16.0) ** 2) / (n / 16.0)).sum())
    assert np.abs(pts[:, 1]).max() == 0.0 and chi2_xy < 44.3, chi2_xy
    # the edge of the table: u0 -> the last face with area, never past it, and a zero-area face is never chosen
    Cz = np.array([0.0, 0.0, 1.0, 1.0, 3.0, 3.0])
    assert list(LR.choose_face(Cz, np.array([0.0, 0.3, 1.0 / 3.0, 0.999999, 1.0]))) == [1, 1, 3, 3, 3]


def test_mesh_pdf_integrates_to_one_over_directions():
    """A closed 80-triangle icosphere seen from outside: every direction into its cone meets two faces and both count. The pdf jumps
    across every projected edge, so the quadrature is a midpoint rule in (cos theta, phi) around the axis to the centre that refines
    itself there: 160 x 160 cells over the cone that holds the mesh, and every cell whose corners and centre do not all meet the same
    set of faces is split into 12 x 12. Within 1e-3 of 1. Counting the first hit only gives the density of the visible half alone."""
    tris = LR.mesh_tris(*icosphere(1), 1.0)
    C = LR.area_table(tris)
    origin = np.array([0.4, -0.3, 3.0])
    axis = -origin / np.linalg.norm(origin)
    q = LR.frame_to_z(axis[None, :])
    mu_min = np.sqrt(1.0 - 1.0 / (origin @ origin)) - 1e-3           # the unit sphere's cone holds the inscribed mesh
    n = 160
    hm, hp = (1.0 - mu_min) / n, 2.0 * np.pi / n

    def dirs(mu, phi):
        st = np.sqrt(np.maximum(0.0, 1.0 - mu * mu))
        return LR.quat_mul((-q[0], -q[1], -q[2], q[3]), np.stack([st * np.cos(phi), st * np.sin(phi), mu], axis=-1))

    def evaluate(mu, phi, **kw):
        return LR.pdf_mesh_from_point(tris, C[-1], origin, dirs(mu.reshape(-1), phi.reshape(-1)), **kw)

    # the regrouped evaluator is the brute force
    rng = np.random.default_rng(2)
    mu_t, phi_t = rng.uniform(mu_min, 1.0, 3000), rng.uniform(0.0, 2.0 * np.pi, 3000)
    brute, hits, risky = LR.pdf_mesh_brute(tris, C[-1], np.tile(origin, (3000, 1)), dirs(mu_t, phi_t))
    np.testing.assert_allclose(evaluate(mu_t, phi_t)[0][~risky], brute[~risky], rtol=1e-9)
    assert set(np.unique(hits)) <= {0, 2}
    total = {}
    for first in (False, True):
        ci, cj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        centre, sig_c = evaluate(mu_min + (ci + 0.5) * hm, (cj + 0.5) * hp, first_hit_only=first)
        gi, gj = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
        sig_g = LR.pdf_mesh_from_point(tris, C[-1], origin, dirs((mu_min + gi * hm).reshape(-1), (gj * hp).reshape(-1)))[1].reshape(n + 1, n + 1)
        sig_c = sig_c.reshape(n, n) if not first else total["sig_c"]
        smooth = (sig_g[:-1, :-1] == sig_c) & (sig_g[1:, :-1] == sig_c) & (sig_g[:-1, 1:] == sig_c) & (sig_g[1:, 1:] == sig_c)
        total["sig_c"] = sig_c
        ri, rj = np.nonzero(~smooth)
        sub = 12 if not first else 3                               # (the first-hit figure is a contrast, not a bound to meet)
        k = (np.arange(sub) + 0.5) / sub
        fine, _ = evaluate(mu_min + (ri[:, None, None] + k[None, :, None]) * hm + 0.0 * k[None, None, :],
                           (rj[:, None, None] + k[None, None, :]) * hp + 0.0 * k[None, :, None], first_hit_only=first)
        total[first] = float(centre.reshape(n, n)[smooth].sum() * hm * hp + fine.sum() * hm * hp / (sub * sub))
        print(f"first hit only = {first}: {n * n} cells, {len(ri)} refined, integral of the mesh pdf over directions {total[first]:.6f}")
    assert abs(total[False] - 1.0) < 1e-3
    assert total[True] < 0.7


def test_sphere_rule_is_a_density():
    """The cone sampler's directions all hit the sphere and its pdf is 1 / (cone's solid angle); inside, 1 / (4 pi)."""
    rng = np.random.default_rng(8)
    n = 20000
    c, r = np.array([0.2, 1.0, -0.3]), 0.7
    o = np.tile([1.5, 0.2, 0.8], (n, 1))
    d = LR.sample_sphere(c, r, o, rng.random(n), rng.random(n))
    p = LR.pdf_sphere(c, r, o, d)
    d2 = ((c - o[0]) ** 2).sum()
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, rtol=1e-14) and (p > 0).mean() > 0.999
    assert np.allclose(p[p > 0], 1.0 / (2.0 * np.pi * (1.0 - np.sqrt(1.0 - r * r / d2))), rtol=1e-12)
    oi = np.tile(c + [0.1, 0.2, -0.3], (n, 1))
    di = LR.sample_sphere(c, r, oi, rng.random(n), rng.random(n))
    assert np.allclose(LR.pdf_sphere(c, r, oi, di), 1.0 / (4.0 * np.pi)) and abs(di.mean(axis=0)).max() < 0.02


def test_probe_ray_sets_leave_almost_nothing_out():
    """For the fixed-seed ray sets of the GPU probe test numpy alone says which rows that test leaves out (a hit with |dot(d, n)| < 1e-6,
    a barycentric coordinate within 1e-9 of an edge): below 1 % for every mesh and placement; and at least 30 % of the kept rows meet two
    or more faces on every closed mesh (the planar mesh cannot be met twice by one ray)."""
    for name in LR.PROBE_MESHES:
        for chained in (False, True):
            c = LR.probe_case(name, chained)
            k = c["keep"]
            m = (c["hits"][k] >= 2).mean()
            print(f"{name} chained={chained}: {len(k)} rays, {1.0 - k.mean():.4%} left out, {m:.1%} of the kept rows with two or more hits")
            assert 1.0 - k.mean() < 0.01
            assert m >= 0.3 or name == "quad"
            assert len(c["sample"]["origins"]) == 4096 and (c["pdf"][k] > 0).mean() > 0.4
