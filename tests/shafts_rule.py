"""Light shafts (pt_scene_set_punctual_media; the rule is in include/pt_amd.h) restated in numpy on top of the rules it composes
— medium_rule (free flight, phase function), medium_grid_rule (delta tracking) and punctual_rule (light evaluation, branch, shadow distance):
the bounce word's layout, the punctual branch at a medium vertex, the resolution of a SHADOW segment through media, a Monte Carlo of the
single-scattering configuration with numpy's own generator, and the quadrature it is held against. Nothing here reads the product."""
from __future__ import annotations

import numpy as np

import medium_rule as MR
import punctual_rule as PR

# ---- the bounce word of a path when both features are in effect (csrc/pt_types.h SHF_*) --------------------------------------------------
BOUNCE_BITS, INDEX_SHIFT, INDEX_BITS, SHADOW_BIT, MEDIUM_SHIFT, MEDIUM_BITS = 8, 8, 11, 19, 20, 12
MAX_DEPTH = (1 << BOUNCE_BITS) - 1            # the host's bound on max_depth
MAX_LIGHTS = 1 << INDEX_BITS                  # 2048
MAX_MEDIUM = 4094                             # the largest medium word: a material handle below 4094, plus 1
SLOT_IDLE = 0xFFFFFFFE                        # the two words that are no path state: every packed word must stay below them


def pack(bounce, medium, shadow, k):
    assert 0 <= bounce <= MAX_DEPTH and 0 <= medium <= MAX_MEDIUM and 0 <= k < MAX_LIGHTS
    return bounce | (medium << MEDIUM_SHIFT) | (((1 << SHADOW_BIT) | (k << INDEX_SHIFT)) if shadow else 0)


def unpack(word):
    """(bounce, medium, shadow, k) — the medium first, as the kernel takes the word apart"""
    medium = word >> MEDIUM_SHIFT
    word &= (1 << MEDIUM_SHIFT) - 1
    return word & ((1 << BOUNCE_BITS) - 1), medium, bool(word & (1 << SHADOW_BIT)), (word >> INDEX_SHIFT) & (MAX_LIGHTS - 1)


# ---- the additions --------------------------------------------------------------------------------------------------------------------
def vertex_throughput(thr, albedo, ph, E, f, n):
    """the punctual branch at a medium vertex: thr' = ((thr * (albedo * ph)) * E) / pm, pm = f / n; ph (m,), E (m, 3)"""
    pm = f / float(n)
    return ((thr * (np.asarray(albedo, dtype=np.float64)[None, :] * ph[:, None])) * E) / pm


def segment_end(t, d_light):
    """t_end = t < D' ? t : D'"""
    return np.where(t < d_light, t, d_light)


def blocked(d, t_end):
    """a free-flight collision at a distance below t_end"""
    return d < t_end


# ---- the single-scattering configuration: an unbounded homogeneous camera medium in front of a black quad at distance T along the ray -----
def single_scatter_quadrature(o, d, T, density, albedo, g, rec, panels, nodes=16):
    """L_c = int_0^T sigma e^(-sigma s) albedo_c ph(dot(d, w(s))) E_c(x(s)) e^(-sigma r(s)) ds by composite Gauss-Legendre: `panels` equal
    panels of `nodes` nodes each. (No occluder stands between the segment and the light: the black quad lies beyond it.)"""
    x, w = np.polynomial.legendre.leggauss(nodes)
    edges = np.linspace(0.0, T, panels + 1)
    h = np.diff(edges) / 2.0
    s = ((edges[:-1] + h)[:, None] + h[:, None] * x[None, :]).reshape(-1)
    ws = (h[:, None] * w[None, :]).reshape(-1)
    X = np.asarray(o, dtype=np.float64)[None, :] + s[:, None] * np.asarray(d, dtype=np.float64)[None, :]
    wl, D, _, E = PR.light_eval(rec, X)
    ph = MR.hg_phase(g, wl @ np.asarray(d, dtype=np.float64))
    f = density * np.exp(-density * s) * ph * np.exp(-density * D)
    return np.asarray(albedo, dtype=np.float64) * ((ws * f)[:, None] * E).sum(axis=0)


def single_scatter_expected(o, d, T, density, albedo, g, rec, panels=2048):
    """(value (3,), relative change when the panels are doubled)"""
    a = single_scatter_quadrature(o, d, T, density, albedo, g, rec, panels)
    b = single_scatter_quadrature(o, d, T, density, albedo, g, rec, 2 * panels)
    den = np.abs(b)
    return b, float(np.max(np.abs(a - b) / np.where(den > 0.0, den, 1.0)))        # (a ray that never enters a spot's cone: 0 both times)


def single_scatter_mc(rng, n, o, d, T, density, albedo, g, rec, f, wall=None):
    """n samples of the rule at max_depth = 2 in that configuration, vectorised over the samples; every draw is numpy's. Returns (n, 3).
    The camera ray (bounce 0) makes its free flight; a vertex in front of the wall reads the selector; below f (no lights list) it takes the
    punctual branch of the one light and becomes a SHADOW segment (bounce 1), whose own free flight over [0, t_end) decides. Everything
    else brings nothing at this depth: the phase branch's next vertex or hit is bounce 2, the wall is black (albedo 0: its punctual
    branch has thr' = 0) and so is the environment. wall(o, w) -> t: the distance at which shadow rays hit the wall (+inf: miss)."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    out = np.zeros((n, 3))
    dist = MR.free_flight(rng.random(n), density)                                # step 1
    vertex = dist < T
    r = rng.random(n)                                                            # the selector: read
    punct = vertex & (PR.branch_of(r, f, False) == 1)
    i = np.nonzero(punct)[0]
    x = o[None, :] + dist[i, None] * d[None, :]
    w, D, d2, E = PR.light_eval(rec, x)                                          # (one light: the index draw has one outcome)
    ph = MR.hg_phase(g, w @ d)
    thr = vertex_throughput(np.ones(3), albedo, ph, E, f, 1)
    alive = ~PR.branch_ends(d2, thr)
    # the SHADOW segment from x (no offset) along w
    dl = PR.shadow_distance(rec, x)
    t = wall(x, w) if wall is not None else np.full(len(i), np.inf)
    t_end = segment_end(t, dl)
    hit = blocked(MR.free_flight(rng.random(len(i)), density), t_end)
    vis = alive & ~hit & PR.visible(t, dl)
    out[i[vis]] = thr[vis]
    return out
