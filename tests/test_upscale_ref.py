"""tests/upscale_ref.py -- the numpy restatement of the upscale stage (EXTENSION) -- held to the properties the
definition promises: the two known answers, non-finite input, linearity in the colour, alpha, the tent without guides, and a
frame whose tier 2 and tier 3 pixels are known.  No GPU and no library."""
import numpy as np
import pytest

import resample_ref
import upscale_ref as u

f32 = np.float32
BAD = [f32(np.nan), f32(-3.0), f32(np.inf), f32(-np.inf), f32(3e38)]


def flat(w, h, rgb, alpha=1.0):
    a = np.empty((h, w, 4), dtype=f32)
    a[..., :3] = f32(rgb)
    a[..., 3] = f32(alpha)
    return a


def test_equal_sizes_return_the_sanitised_mean():
    color = u.make_frame(45, 35, seed=9)
    alb, nor, dep = u.make_guides(45, 35, seed=9, poison=False)
    want = u.sanitise(color, 3, 65536.0)
    out, det = u.upscale(color, 3, 45, 35, lo=(alb, None, dep), hi=(alb, None, dep), details=True)
    assert np.array_equal(out[..., :3], want[..., :3]) and np.array_equal(out[..., 3], color[..., 3])
    assert det["counts"] == (0, 0, 45 * 35)
    # with the normal pair n . n can be 1 - ulp, and its 8th power a few ulps below 1: w1 is then not exactly 1
    out, det = u.upscale(color, 3, 45, 35, lo=(alb, nor, dep), hi=(alb, nor, dep), details=True)
    assert u.ulps(out[..., :3], want[..., :3]).max() <= 16 and det["counts"][:2] == (0, 0)
    # no pair at all: a bilinear resize at ratio 1 is the identity
    assert np.array_equal(u.upscale(color, 3, 45, 35)[..., :3], want[..., :3])


def step_frames(e):
    """An 8 x 8 lo frame and the 16 x 16 hi guides of a vertical step at hi column e: value 1, albedo 0.8, depth 0.2 left of it,
    value 100, albedo 0.1, depth 0.6 from it on; every lo texel is the mean of its two hi columns."""
    left = np.arange(16) < e
    value, albedo, depth = np.where(left, 1.0, 100.0), np.where(left, 0.8, 0.1), np.where(left, 0.2, 0.6)
    hi = [np.broadcast_to(flat(1, 1, 0.0)[0], (16, 16, 4)).copy() for _ in range(3)]
    lo = [flat(8, 8, 0.0) for _ in range(3)]
    for frame, small, v in zip(hi, lo, (value, albedo, depth)):
        frame[..., :3] = v.astype(f32)[None, :, None]
        small[..., :3] = ((v[0::2] + v[1::2]) * 0.5).astype(f32)[None, :, None]
    return (lo[0], lo[1], lo[2]), (hi[1], hi[2]), np.broadcast_to(value[None, :], (16, 16))


@pytest.mark.parametrize("e,bound", [(6, 0.00005), (8, 0.00005), (7, 0.0033), (9, 0.0033)])
def test_step_stays_a_step(e, bound):
    """Known answer: every output pixel is within 0.005 % (the edge between texels) or 0.33 % (the edge through a texel) of the
    step of its own side's value, where the tent leaves a quarter of the step and more next to the edge."""
    (color, lo_a, lo_z), (hi_a, hi_z), own = step_frames(e)
    out = u.upscale(color, 1, 16, 16, lo=(lo_a, None, lo_z), hi=(hi_a, None, hi_z))
    err = np.abs(out[..., 0].astype(np.float64) - own) / 99.0
    print(f"e = {e}: the largest error is {err.max():.3e} of the step")
    assert err.max() <= bound
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    tent = resample_ref.resample(color, 1, 16, 16, filter=resample_ref.TENT)
    worst = (np.abs(tent[..., 0].astype(np.float64) - own) / 99.0).max()
    assert 0.25 <= worst <= 0.75


@pytest.mark.parametrize("target", ["colour", "albedo", "normal", "depth"])
def test_non_finite_input_gives_finite_output(target):
    k = ["colour", "albedo", "normal", "depth"].index(target)
    for shape in ((8, 8, 16, 16), (5, 3, 7, 9), (6, 6, 6, 6)):
        w, h, W, H = shape
        color = u.make_frame(w, h, seed=4, poison=False)
        lo, hi = u.coherent_pair(w, h, W, H, seed=4, poison=False)
        for n, bad in enumerate(BAD):
            for side in ((0, 1) if k else (0,)):
                c, l, g = color.copy(), [x[0].copy() for x in lo], [x[0].copy() for x in hi]
                victim = c if k == 0 else (l, g)[side][k - 1]
                victim.reshape(-1, 4)[n::3, (n + side) % 3] = bad
                victim[0, 0, :3] = bad
                out = u.upscale(c, 1, W, H, lo=tuple(l), hi=tuple(g))
                assert np.isfinite(out).all(), (target, shape, bad, side)


def test_twice_the_colour_is_twice_the_result():
    """The weights do not see the colour, and a factor of two is exact in every product, sum and quotient below the cap."""
    color = u.make_frame(16, 17, seed=2, poison=False)
    color[..., :3] = np.minimum(color[..., :3], f32(1000.0))
    lo, hi = u.coherent_pair(16, 17, 45, 35, seed=2, poison=False)
    double = color.copy()
    double[..., :3] *= f32(2.0)
    for mask in (0, 5, 7):
        a = u.upscale(color, 1, 45, 35, lo=u.subset(lo, mask), hi=u.subset(hi, mask))
        b = u.upscale(double, 1, 45, 35, lo=u.subset(lo, mask), hi=u.subset(hi, mask))
        assert np.array_equal(b[..., :3], a[..., :3] * f32(2.0)) and np.array_equal(a[..., 3], b[..., 3])


def test_alpha_one_in_is_alpha_one_out():
    color = u.make_frame(16, 17, seed=3)
    color[..., 3] = f32(1.0)
    lo, hi = u.coherent_pair(16, 17, 45, 35, seed=3)
    assert (u.upscale(color, 4, 45, 35, lo=lo, hi=hi)[..., 3] == 1.0).all()
    # and otherwise it is the nearest texel's, neither filtered nor divided by the count
    color = u.make_frame(3, 5, seed=3)
    _, _, nx = u.axis_table(3, 7)
    _, _, ny = u.axis_table(5, 9)
    assert np.array_equal(u.upscale(color, 4, 7, 9)[..., 3], color[ny[:, None], nx[None, :], 3])


@pytest.mark.parametrize("w,h,W,H", [(8, 8, 16, 16), (16, 17, 45, 35), (3, 5, 7, 9), (2, 2, 64, 64), (64, 36, 128, 72), (1, 1, 5, 3)])
def test_without_guides_it_is_the_tent(w, h, W, H):
    """No pair: the weights are the tent's of the resample stage, normalised at the end (A0 / D0) instead of in the table, and
    taken as products of two axes instead of pass by pass.  All terms are non-negative, so every rounding costs at most 2^-24 of
    the result: here two table weights, their product, the product with the colour and four non-zero sums for A0, the same less
    one for D0, and the quotient, 16 in all; there a table weight, a product and two sums per pass, 8 in all.  24 half-ulps are
    12 ulps, up to 24 where the result sits just above a power of two: the bound is 32.  Measured: 3 at most."""
    color = u.make_frame(w, h, seed=W)
    got = u.upscale(color, 3, W, H)
    want = resample_ref.resample(color, 3, W, H, filter=resample_ref.TENT)
    d = u.ulps(got[..., :3], want[..., :3]).max()
    print(f"{w}x{h} -> {W}x{H}: {d} ulps from the tent")
    assert d <= 32 and np.array_equal(got[..., 3], want[..., 3])


def test_known_pixels_take_tier_two_and_three():
    """8 x 8 -> 16 x 16 with the normal pair alone.  Every lo texel is a hit but (2, 2), every hi pixel a hit but four misses,
    which match a lo miss only: (4, 4) has texel (2, 2) in its 2 x 2 footprint (tier 1); (7, 7) and (7, 4) have it in their
    4 x 4 footprint only -- output column 7 takes the texels 2 .. 5, narrow weights on 3 and 4 -- (tier 2); (12, 12) has no
    miss within reach (tier 3: plain bilinear)."""
    color = u.make_frame(8, 8, seed=6, poison=False)
    lo_n, hi_n = flat(8, 8, 0.0), flat(16, 16, 0.0)
    lo_n[..., 2] = hi_n[..., 2] = f32(1.0)
    lo_n[2, 2, :3] = 0.0
    for x, y in ((4, 4), (7, 7), (7, 4), (12, 12)):
        hi_n[y, x, :3] = 0.0
    out, det = u.upscale(color, 1, 16, 16, lo=(None, lo_n, None), hi=(None, hi_n, None), details=True)
    tier = det["tier"]
    assert {(x, y) for y, x in np.argwhere(tier == 2)} == {(7, 7), (7, 4)}
    assert {(x, y) for y, x in np.argwhere(tier == 3)} == {(12, 12)}
    assert det["counts"] == (2, 1, 256) and tier[4, 4] == 1
    mean = u.sanitise(color, 1, 65536.0)
    # the one match: (w * c) / w, a rounded product over its own factor
    assert u.ulps(out[4, 4, :3], mean[2, 2, :3]).max() <= 1 and u.ulps(out[7, 7, :3], mean[2, 2, :3]).max() <= 1
    plain = u.upscale(color, 1, 16, 16)
    assert np.array_equal(out[12, 12], plain[12, 12]) and not np.array_equal(out[7, 7], plain[7, 7])
