"""Adaptive sampling, host side (no GPU): the round schedule of pt_render_adaptive and its argument checks."""
import ctypes

import numpy as np
import pytest


def schedule_py(m, n):
    """include/pt_amd.h: b_0 = 0, b_1 = m/2, b_2 = m, b_{i+1} = min(N, b_i + max(m/2, b_i/2)), integer divisions."""
    b = [0, m // 2, m]
    while b[-1] < n:
        b.append(min(n, b[-1] + max(m // 2, b[-1] // 2)))
    return b


@pytest.mark.parametrize("m,n", [(2, 2), (2, 9), (16, 4000), (64, 100), (7, 7)])
def test_schedule_matches_the_stated_rule(pt, m, n):
    got = pt.adaptive_schedule(m, n)
    assert got == schedule_py(m, n)
    assert got[0] == 0 and got[-1] == n and all(a < b for a, b in zip(got, got[1:]))


def test_schedule_of_the_headline_frame_has_sixteen_rounds(pt):
    assert len(pt.adaptive_schedule(16, 4000)) - 1 == 16


def test_schedule_cap_writes_a_prefix_and_returns_the_full_count(pt):
    full = schedule_py(16, 4000)
    buf = (ctypes.c_uint32 * 5)()
    assert pt.lib.pt_adaptive_schedule(16, 4000, buf, 5) == len(full)
    assert list(buf) == full[:5]
    assert pt.lib.pt_adaptive_schedule(16, 4000, None, 0) == len(full)


@pytest.mark.parametrize("m,n,what", [(1, 8, "min_spp"), (0, 8, "min_spp"), (8, 7, "max_spp")])
def test_schedule_rejects_bad_arguments(pt, m, n, what):
    assert pt.lib.pt_adaptive_schedule(m, n, None, 0) == -1
    assert what in pt.lib.pt_last_error().decode()
    with pytest.raises(pt.PtError, match=what):
        pt.adaptive_schedule(m, n)


def test_adaptive_entry_points_are_declared_and_bound(pt):
    for name in ("pt_render_pixels", "pt_adaptive_schedule", "pt_render_adaptive", "pt_resolve_u8_counts"):
        assert name in pt.ABI_SYMBOLS and hasattr(pt.lib, name)
    # the options struct as the header lays it out: two u32, a double, two u32, a pointer
    assert ctypes.sizeof(pt.AdaptiveOpts) == 32 and pt.AdaptiveOpts.threshold.offset == 8 and pt.AdaptiveOpts.stream.offset == 24


# ---- the numpy restatement of the rule (tests/adaptive_rule.py), against outcomes worked out by hand ---------------------------------------
# A 5 x 4 frame, min 4, max 16, threshold 0.5: the bounds are 0 2 4 6 9 13 16, so the tests come after rounds 1, 2, 3 and 4.
RULE_W, RULE_H, RULE_M, RULE_N, RULE_THR = 5, 4, 4, 16, 0.5


def _synthetic(value):
    """render_range of a frame whose pixel (y, x) returns value(y, x, round) per sample and channel in every sample of a round."""
    from adaptive_rule import schedule
    b, calls = schedule(RULE_M, RULE_N), []

    def render_range(lo, hi):
        calls.append((lo, hi))
        i = b.index(lo)
        assert b[i + 1] == hi
        out = np.empty((RULE_H, RULE_W, 3))
        for y in range(RULE_H):
            for x in range(RULE_W):
                out[y, x, :] = value(y, x, i) * (hi - lo)
        return out

    return render_range, calls


def test_rule_module_schedule_is_the_librarys(pt):
    from adaptive_rule import schedule
    for m, n in [(4, 16), (4, 12), (5, 40), (2, 9), (6, 7), (8, 8), (4, 32)]:
        assert schedule(m, n) == pt.adaptive_schedule(m, n)
    assert schedule(RULE_M, RULE_N) == [0, 2, 4, 6, 9, 13, 16] and schedule(4, 12) == [0, 2, 4, 6, 9, 12]


def test_replay_isolated_bad_corner_pixel_keeps_its_three_neighbours():
    """Every pixel returns 1 per sample, so A = B = 1 and the error is 0, but pixel (0, 0) returns 2 in round 0. Its two means are then
    test 1 (n_E 2, n_O 2): A 2,    B 1, d 3,    M 18/4:  3 / (1e-4 + 2.1213)    = 1.414  bad
    test 2 (n_E 4, n_O 2): A 1.5,  B 1, d 1.5,  M 24/6:  1.5 / 2.0001           = 0.750  bad
    test 3 (n_E 4, n_O 5): A 1.5,  B 1, d 1.5,  M 33/9:  1.5 / (1e-4 + 1.9149)  = 0.783  bad
    test 4 (n_E 8, n_O 5): A 1.25, B 1, d 0.75, M 45/13: 0.75 / (1e-4 + 1.8605) = 0.403  below 0.5
    so it stops in round 4 with 13 samples and the sum 15; (0, 1), (1, 0) and (1, 1), never bad themselves, go with it and stop with 13
    samples and the sum 13; all others stop at the first test with 4."""
    from adaptive_rule import adaptive_replay
    rr, calls = _synthetic(lambda y, x, i: 2.0 if (y, x, i) == (0, 0, 0) else 1.0)
    acc, counts, rounds = adaptive_replay(rr, RULE_H, RULE_W, RULE_M, RULE_N, RULE_THR)
    want_counts = np.full((RULE_H, RULE_W), 4, dtype=np.uint32)
    want_counts[:2, :2] = 13
    want_rounds = np.full((RULE_H, RULE_W), 1)
    want_rounds[:2, :2] = 4
    want_acc = np.repeat(want_counts[..., None].astype(np.float64), 3, axis=2)
    want_acc[0, 0, :] = 15.0
    assert counts.dtype == np.uint32
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(rounds, want_rounds)
    np.testing.assert_array_equal(acc, want_acc)
    assert calls == [(0, 2), (2, 4), (4, 6), (6, 9), (9, 13)]                    # nobody is left for the last round


def test_replay_nan_pixel_never_stops_and_neither_do_its_neighbours():
    from adaptive_rule import adaptive_replay
    rr, calls = _synthetic(lambda y, x, i: np.nan if (y, x, i) == (2, 2, 0) else 1.0)
    acc, counts, rounds = adaptive_replay(rr, RULE_H, RULE_W, RULE_M, RULE_N, RULE_THR)
    want_counts = np.full((RULE_H, RULE_W), 4, dtype=np.uint32)
    want_counts[1:4, 1:4] = 16                                                   # rows 1-3 and columns 1-3: the pixel and its eight neighbours
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(rounds, np.where(want_counts == 16, -1, 1))
    assert np.isnan(acc[2, 2]).all() and np.isfinite(np.delete(acc.reshape(-1, 3), 2 * RULE_W + 2, axis=0)).all()
    np.testing.assert_array_equal(np.delete(acc[..., 0].reshape(-1), 2 * RULE_W + 2), np.delete(want_counts.reshape(-1), 2 * RULE_W + 2))
    assert calls == [(0, 2), (2, 4), (4, 6), (6, 9), (9, 13), (13, 16)]
    # ... under every threshold that is a number, and a NaN threshold stops nobody at all
    for thr, everyone in ((np.inf, False), (1e30, False), (np.nan, True)):
        _, c, _ = adaptive_replay(_synthetic(lambda y, x, i: np.nan if (y, x, i) == (2, 2, 0) else 1.0)[0], RULE_H, RULE_W, RULE_M, RULE_N, thr)
        np.testing.assert_array_equal(c, np.full_like(want_counts, 16) if everyone else want_counts)


def test_replay_frame_of_zeros_stops_everywhere_at_the_first_test():
    from adaptive_rule import adaptive_replay, schedule
    rr, calls = _synthetic(lambda y, x, i: 0.0)
    acc, counts, rounds = adaptive_replay(rr, RULE_H, RULE_W, RULE_M, RULE_N, RULE_THR)
    assert (counts == schedule(RULE_M, RULE_N)[2]).all() and (counts == 4).all() and (rounds == 1).all() and (acc == 0.0).all()
    assert calls == [(0, 2), (2, 4)]
    # threshold <= 0: 0 < 0 is false, nobody stops
    _, counts, rounds = adaptive_replay(_synthetic(lambda y, x, i: 0.0)[0], RULE_H, RULE_W, RULE_M, RULE_N, 0.0)
    assert (counts == RULE_N).all() and (rounds == -1).all()


def test_rule_module_dilate_and_tiled_index():
    from adaptive_rule import dilate, tiled_index
    bad = np.zeros((4, 5), dtype=bool)
    bad[0, 0] = bad[3, 2] = True
    want = np.array([[1, 1, 0, 0, 0], [1, 1, 0, 0, 0], [0, 1, 1, 1, 0], [0, 1, 1, 1, 0]], dtype=bool)
    np.testing.assert_array_equal(dilate(bad), want)
    t = tiled_index(9, 10)                                                       # 2 x 2 tiles, the right column and the bottom row ragged
    assert t[0, 0] == 0 and t[0, 7] == 7 and t[1, 0] == 8 and t[7, 7] == 63 and t[0, 8] == 64 and t[0, 9] == 65 and t[8, 0] == 128 and t[8, 9] == 193
    assert len(np.unique(t)) == 90
