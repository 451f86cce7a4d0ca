"""bt_debug_upscale_host -- the whole upscale stage (EXTENSION) on the host through csrc/bt_upscale.hpp's own
functions -- against tests/upscale_ref.py, bit for bit and count for count, and the handle's tables against numpy's.  No GPU."""
import numpy as np
import pytest

import upscale_ref as u

f32 = np.float32
# (w, h, W, H): one texel, one texel spread, odd ratios, 2 : 1, 4 : 1, 32 : 1, more than one tile with a ragged edge, one column or
# row into a second tile, equal sizes, the interactive case
SHAPES = [(1, 1, 1, 1), (1, 1, 5, 3), (3, 5, 7, 9), (8, 8, 16, 16), (8, 8, 32, 32), (2, 2, 64, 64), (16, 17, 45, 35), (17, 16, 33, 33),
          (45, 35, 45, 35), (64, 36, 128, 72)]
OTHER = dict(sigma_depth=0.3, sigma_albedo=0.03, normal_squarings=0, min_weight=0.1, max_value=100.0)


def settings():
    """(colour count, (albedo, normal, depth) counts, parameters): counts {1, 3} x {1, 4}, two parameter sets."""
    return [(1, (1, 1, 1), {}), (3, (4, 4, 4), OTHER), (3, (1, 4, 1), {}), (1, (4, 1, 4), dict(OTHER, normal_squarings=6))]


def frames(w, h, W, H, counts, coherent):
    """-> (colour sums, lo guides, hi guides), poisoned at the first pixel, the last one and pixel 256."""
    seed = w * 1000 + h + W
    color = u.make_frame(w, h, seed=seed)
    if coherent:
        lo, hi = u.coherent_pair(w, h, W, H, seed=seed, samples=counts)
    else:
        lo, hi = u.make_guides(w, h, seed=seed, samples=counts), u.make_guides(W, H, seed=seed + 1, samples=counts)
    return color, lo, hi


def cases(w, h, W, H):
    """Every subset of guide pairs under every setting, on random and on coherent guides."""
    for n, (samples, counts, p) in enumerate(settings()):
        color, lo, hi = frames(w, h, W, H, counts, coherent=n % 2 == 0)
        for mask in range(8):
            yield color, samples, u.subset(lo, mask), u.subset(hi, mask), p


@pytest.mark.parametrize("w,h,W,H", SHAPES)
def test_host_is_the_restatement(bendy, w, h, W, H):
    tiers = np.zeros(4, dtype=np.int64)
    for color, samples, lo, hi, p in cases(w, h, W, H):
        got, st = bendy.upscale_host(color, samples, W, H, lo=lo, hi=hi, stats=True, **p)
        want, det = u.upscale(color, samples, W, H, lo=lo, hi=hi, details=True, **{**u.DEFAULTS, **p})
        assert np.array_equal(got, want), (p, samples, np.argwhere(got != want)[:4])          # no pixel is exempt
        assert (st.tier2, st.tier3, st.pixels) == det["counts"], (p, samples)
        assert np.isfinite(got[..., :3]).all()
        tiers += np.bincount(det["tier"].ravel(), minlength=4)
    if W * H >= 256:
        assert tiers[1] > 0 and tiers[2] > 0 and tiers[3] > 0                                 # every tier was taken somewhere


@pytest.mark.parametrize("w,h,W,H", SHAPES + [(1, 3, 1, 257), (3, 1, 257, 1), (7, 7, 1000, 7)])
def test_tables_are_numpys(bendy, w, h, W, H):
    handle = bendy.Upscale()
    handle.host(np.ones((h, w, 4), dtype=f32), 1, W, H)
    for axis, (src, dst) in enumerate(((w, W), (h, H))):
        first, weights, nearest = handle.weights(axis)
        rf, rw, rn = u.axis_table(src, dst)
        assert np.array_equal(first, rf) and np.array_equal(weights, rw) and np.array_equal(nearest, rn)
        assert weights.shape == (dst, 8) and np.array_equal(handle.weights("xy"[axis])[1], weights)
        # the narrow weights are the bilinear pair and sum to 1; a tile's 16 outputs stay within 19 source texels
        assert np.allclose(weights[:, :4].sum(axis=1), 1.0, atol=1e-6) and (np.diff(first) >= 0).all()
        for i0 in range(0, dst, 16):
            i1 = min(i0 + 16, dst) - 1
            assert first[i1] + 3 - first[i0] + 1 <= 19


def test_handle_keeps_and_replaces_its_tables(bendy):
    handle = bendy.Upscale(sigma_depth=0.3)
    color, lo, hi = frames(16, 17, 45, 35, (1, 1, 1), True)
    a = handle.host(color, 1, 45, 35, lo=lo, hi=hi)
    assert np.array_equal(a, u.upscale(color, 1, 45, 35, lo=lo, hi=hi, **{**u.DEFAULTS, "sigma_depth": 0.3}))
    small = u.make_frame(1, 1, seed=3)
    assert np.array_equal(handle.host(small, 1, 5, 3), u.upscale(small, 1, 5, 3))
    assert handle.weights(0)[0].shape == (5,)
    assert np.array_equal(handle.host(color, 1, 45, 35, lo=lo, hi=hi), a)
    assert np.array_equal(bendy.upscale_host(color, 1, 45, 35, lo=lo, hi=hi, sigma_depth=0.3), a)
    with pytest.raises(bendy.BendyError):
        bendy.Upscale().weights(0)                                   # no call, no table


def test_equal_sizes_return_the_sanitised_mean(bendy):
    """Known answer: same frames as lo and hi guides, no normal pair -> the sanitised mean bit for bit, both counts 0."""
    color = u.make_frame(45, 35, seed=9)
    g = u.make_guides(45, 35, seed=9, poison=False)
    pair = (g[0], None, g[2])
    got, st = bendy.upscale_host(color, 3, 45, 35, lo=pair, hi=pair, stats=True)
    want = u.sanitise(color, 3, 65536.0)
    assert np.array_equal(got[..., :3], want[..., :3]) and np.array_equal(got[..., 3], color[..., 3])
    assert (st.tier2, st.tier3, st.pixels) == (0, 0, 45 * 35)
