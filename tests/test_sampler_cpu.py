"""The Sobol sampler (pt_scene_set_sampler), host side (no GPU): the numpy restatement of the rule
(tests/sampler_rule.py) is a (0,2)-sequence per pair under every scramble tried, the library exports the entry points, and the CLI
refuses an unknown sampler before it opens a device."""
import os
import subprocess

import numpy as np

import sampler_rule as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "thu-acg-f2024-path-tracer_amd", "pt_render")


def test_elementary_intervals_hold_one_point_each():
    """For every m in 0..10 and blocks [a 2^m, (a+1) 2^m), a in {0, 1, 3, 5}, the 2^m points of a pair put exactly one point into
    every elementary interval 2^-p x 2^-(m-p), p = 0..m — under 40 random key triples, index shuffle included. Zero violations."""
    rng = np.random.default_rng(1)
    bad = 0
    for _ in range(40):
        k0, k1, k2 = (int(v) for v in rng.integers(0, 2 ** 32, 3))
        for m in range(11):
            for a in (0, 1, 3, 5):
                s = np.arange(a << m, (a + 1) << m, dtype=np.uint64)
                x, y = R.pair_points(s, k0, k1, k2)
                bad += R.elementary_interval_violations(x, y, m)
    assert bad == 0


def test_whole_rule_keeps_the_property_per_pixel_and_pair():
    """The same property on the values the kernels consume (keys from the Philox block, top 32 bits of the 64-bit value)."""
    for seed, pixel, pair in ((1, 0, 0), (7, 4095, 3), ((5 << 32) | 9, 123456, 17)):
        for m in (0, 3, 6, 9):
            s = np.arange(3 << m, 4 << m, dtype=np.uint64)
            x = R.sobol_u64(seed, pixel, s, 2 * pair) >> np.uint64(32)
            y = R.sobol_u64(seed, pixel, s, 2 * pair + 1) >> np.uint64(32)
            assert R.elementary_interval_violations(x, y, m) == 0


def test_five_step_sobol1_is_the_direction_number_loop():
    rng = np.random.default_rng(2)
    i = np.concatenate([rng.integers(0, 2 ** 32, 200000, dtype=np.uint64), np.arange(70000, dtype=np.uint64)])
    np.testing.assert_array_equal(R.sobol1(i), R.sobol1_loop(i))


def test_pairs_and_pixels_are_shuffled_differently():
    s = np.arange(64, dtype=np.uint64)
    base = R.sobol_u64(3, 10, s, 0)
    other_pair = R.sobol_u64(3, 10, s, 2)
    other_pixel = R.sobol_u64(3, 11, s, 0)
    other_seed = R.sobol_u64(3 | (1 << 32), 10, s, 0)
    for other in (other_pair, other_pixel, other_seed):
        assert (base != other).all()
        # not the same point set in another order either: the shuffles and the scrambles both differ
        assert len(np.intersect1d(base >> np.uint64(32), other >> np.uint64(32))) < 4
    # and the order in which a stratum sequence is visited differs: the 1-D strata of 16 points
    order = lambda v: tuple(np.argsort(v[:16]))
    assert order(base) != order(other_pair) and order(base) != order(other_pixel)
    # the two components of a pair are different coordinates, the filler words differ from the points
    assert (R.sobol_u64(3, 10, s, 0) != R.sobol_u64(3, 10, s, 1)).all()
    assert ((base >> np.uint64(32)) != (base & R.M)).all()


def test_numpy_philox_is_the_oracles(orc):
    rng = np.random.default_rng(3)
    for _ in range(50):
        c = [int(v) for v in rng.integers(0, 2 ** 32, 4)]
        k = [int(v) for v in rng.integers(0, 2 ** 32, 2)]
        assert [int(v) for v in R.philox4x32_10(*c, *k)] == orc.philox4x32_10(c, k)
    # kind 0's value is the draw the oracle's generator makes
    for seed, pixel, s, d in ((1, 2, 3, 0), (9, 77, 4100, 5), ((3 << 32) | 5, 1000, 12, 62)):
        assert R.unit(R.independent_u64(seed, pixel, s, d)) == orc.rng_uniform(seed, pixel, s, d)


def test_sampler_symbols_exported(pt):
    for name in ("pt_scene_set_sampler", "pt_scene_sampler", "pt_sampler_probe"):
        assert name in pt.ABI_SYMBOLS and hasattr(pt.lib, name), name
    assert pt.SAMPLERS == {"independent": 0, "sobol": 1}


def test_cli_refuses_unknown_sampler():
    for bad in ("bogus", "1", ""):
        r = subprocess.run([EXE, "-s", "3", "--width", "16", "--spp", "1", "--sampler", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
        assert "--sampler" in r.stderr


def test_cli_usage_names_the_sampler():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--sampler independent|sobol" in r.stdout
