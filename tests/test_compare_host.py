"""bt_debug_compare_host -- the whole compare stage (EXTENSION) on the host through csrc/bt_compare.hpp's own
functions -- against tests/compare_ref.py: `==` on every float64 stat, array_equal on the three planes, psnr to rtol 1e-12, the
tail at three fractions.  No pixel is exempt.  No GPU."""
import math

import numpy as np
import pytest

import compare_ref as c

# one pixel, one row / column inside a tile, a frame smaller than the window, one tile, one column / row into a second tile, 3 x 3
# tiles with a ragged edge, the interactive shapes
SHAPES = [(1, 1), (5, 1), (1, 5), (11, 11), (16, 16), (17, 16), (16, 17), (33, 33), (45, 35), (64, 36)]
TAILS = (0.01, 0.5, 1.0)


def cases(w, h):
    """(X, Y, n_x, n_y, parameters): noise {0, 0.05, 0.8} x the three kinds of spots, counts {1, 3} x {1, 4}, epsilon {0.01, 1e-4}."""
    counts = [(1, 1), (3, 4), (3, 1), (1, 4)]
    n = 0
    for noise in (0.0, 0.05, 0.8):
        for poison in (None, "nonfinite", "big"):
            nx, ny = counts[n % 4]
            p = dict(epsilon=1e-4, peak=2.0) if n % 2 else {}
            X, Y = c.make_pair(w, h, seed=w * 1000 + h * 10 + n, noise=noise, nx=nx, ny=ny, poison=poison)
            yield X, Y, nx, ny, p
            n += 1


def check_stats(st, want):
    for k in c.FIELDS:
        got = getattr(st, k)
        if k == "psnr":
            assert (got == want[k]) if math.isinf(want[k]) else math.isclose(got, want[k], rel_tol=1e-12), (k, got, want[k])
        else:
            assert got == want[k], (k, got, want[k])


@pytest.mark.parametrize("w,h", SHAPES)
def test_host_is_the_restatement(bendy, w, h):
    seen_bad = seen_cap = 0
    for X, Y, nx, ny, p in cases(w, h):
        st, E, V, S, tails = bendy.compare_host(X, Y, nx, ny, tail=TAILS, **p)
        want = c.measure(X, Y, nx, ny, **{**c.DEFAULTS, **p})
        check_stats(st, want)
        assert np.array_equal(E, want["E"]) and np.array_equal(np.signbit(E), np.signbit(want["E"]))
        assert np.array_equal(V, want["v"]) and np.array_equal(S, want["s"])
        assert np.isfinite(S).all() and np.isfinite(E).all() and math.isfinite(st.mse) and math.isfinite(st.rel_mse) and math.isfinite(st.ssim)
        for f, got in zip(TAILS, tails):
            assert got == c.tail(want["E"], f), f
        seen_bad += st.nonfinite
        seen_cap += int((E == c.FLT_MAX).sum())
    assert seen_bad >= 2                   # the non-finite spots were counted
    if w * h > 1:
        assert seen_cap >= 1               # and a 3e38 against a small value reached the cap of the error plane


def test_host_entry_point_refuses_the_same(bendy):
    ones = np.ones((4, 4, 4), dtype=np.float32)
    for kw, word in ((dict(test_samples=0), "0 samples"), (dict(reference_samples=0), "0 samples"), (dict(epsilon=0.0), ".epsilon"),
                     (dict(epsilon=float("nan")), ".epsilon"), (dict(peak=-1.0), ".peak"), (dict(peak=float("inf")), ".peak"),
                     (dict(tail=(0.0,)), "fraction"), (dict(tail=(0.5, 1.5)), "fraction")):
        with pytest.raises(bendy.BendyError) as e:
            bendy.compare_host(ones, ones, **kw)
        assert e.value.code == -1 and word in str(e.value), (kw, str(e.value))
    with pytest.raises(bendy.BendyError):
        bendy.compare_host(ones, np.ones((4, 5, 4), dtype=np.float32))
