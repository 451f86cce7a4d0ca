"""The numpy restatement of the glare stage (tests/glare_ref.py; EXTENSION) against its own properties: what the
definition promises, checked without the library.  test_glare_host.py then holds the library's per-texel code to it."""
import numpy as np
import pytest

import glare_ref as g

f32 = np.float32
SHAPES = [(1, 1), (2, 1), (1, 2), (3, 5), (16, 17), (45, 35), (257, 3), (300, 200)]          # width x height


def test_effective_levels():
    assert [g.effective_levels(10, w, h) for w, h in SHAPES] == [0, 1, 1, 3, 5, 6, 9, 9]
    assert [g.effective_levels(2, w, h) for w, h in SHAPES] == [0, 1, 1, 2, 2, 2, 2, 2]
    assert g.effective_levels(16, 65536, 1) == 16 and g.effective_levels(16, 65537, 1) == 16 and g.effective_levels(0, 300, 200) == 0


def test_weights():
    assert g.level_weights(1, 7.0) == [f32(1.0)]
    assert g.level_weights(4, 1.0) == [f32(0.25)] * 4
    assert g.level_weights(3, 2.0) == [f32(1 / 7), f32(2 / 7), f32(4 / 7)]
    w = g.level_weights(16, 0.5)
    assert all(isinstance(v, f32) for v in w) and abs(sum(float(v) for v in w) - 1.0) < 16 * 2.0 ** -24


@pytest.mark.parametrize("levels", [1, 3, 6, 10])
def test_constant_frame_comes_back(levels):
    """Down and up are exact on a constant; only the L products and L - 1 sums of step 5 and the composite round."""
    for w, h in SHAPES:
        L = g.effective_levels(levels, w, h)
        for v in (f32(0.3), f32(1.0), f32(137.25), f32(2.0 ** -18 * 3)):
            frame = np.empty((h, w, 4), dtype=f32)
            frame[..., :3] = v
            frame[..., 3] = 0.5
            out, planes = g.glare(frame, 1, levels=levels, spread=1.5, strength=1.0, planes=True)
            assert len(planes) == L
            d = int(g.ulps(out[..., :3], v).max())
            assert d <= 2 * L + 1, (w, h, levels, float(v), d)
            assert np.array_equal(out[..., 3], frame[..., 3])
            for a in planes:                                   # a constant plane at every level
                assert (a[..., :3] == a[0, 0, 0]).all() and not a[..., 3].any()


def _impulse():
    f = np.zeros((256, 256, 4), dtype=f32)
    f[..., 3] = 1.0
    f[128, 131, :3] = (100.0, 50.0, 25.0)
    return f


@pytest.mark.parametrize("levels, count", [(1, 36), (2, 196)])
def test_impulse_keeps_its_energy_exactly(levels, count):
    out = g.glare(_impulse(), 1, levels=levels, spread=1.0, strength=1.0)
    for ch in range(3):
        assert int((out[..., ch] != 0).sum()) == count
    assert float(out[..., 0].astype(np.float64).sum()) == 100.0
    assert (out[..., :3] >= 0).all()


@pytest.mark.parametrize("levels", [3, 4])
def test_impulse_keeps_its_energy(levels):
    """Fewer than a hundred roundings of 2^-24 on non-negative terms."""
    out = g.glare(_impulse(), 1, levels=levels, spread=1.0, strength=1.0)
    total = float(out[..., 0].astype(np.float64).sum())
    print(f"levels {levels}: relative energy error {abs(total - 100.0) / 100.0:.3g}")
    assert abs(total - 100.0) / 100.0 <= 1e-5
    assert (out[..., :3] >= 0).all()


def test_sanitising():
    a = g.make_frame(45, 35, seed=3, poison=False)
    bad = [f32(np.nan), f32(-3.0), f32(-np.inf), f32(np.inf), f32(3e38)]
    for n, (y, x) in enumerate([(0, 0), (34, 44), (5, 31), (17, 20), (20, 17), (33, 1)]):
        for ch in range(3):
            a[y, x, ch] = bad[(n + ch) % 5]
    assert not np.isfinite(a[..., :3]).all()
    s = g.sanitise(a, 3, 65536.0)
    assert np.isfinite(s).all() and (s >= 0).all() and (s <= 65536.0).all()
    assert s[0, 0, 0] == 0 and s[0, 0, 1] == 0 and s[0, 0, 2] == 0          # NaN, -3, -inf
    assert s[34, 44, 2] == 65536.0 and s[5, 31, 1] == 65536.0                 # +inf, then 3e38 / 3
    for levels in (0, 1, 6):
        out = g.glare(a, 3, levels=levels)
        assert np.isfinite(out[..., :3]).all() and np.array_equal(out[..., 3], a[..., 3])


def test_strength_zero_returns_the_sanitised_mean():
    a = g.make_frame(45, 35, seed=4)
    out = g.glare(a, 3, levels=6, strength=0.0)
    assert np.array_equal(out[..., :3], g.sanitise(a, 3, 65536.0)[..., :3])
    assert np.array_equal(g.glare(a, 3, levels=0, strength=1.0), out)


def test_linear_in_exact_scaling():
    a = g.make_frame(45, 35, seed=5, poison=False)
    a[..., :3] = np.minimum(a[..., :3], f32(8192.0))          # 2 * mean stays below the cap
    for levels in (1, 3, 6):
        one = g.glare(a, 1, levels=levels, spread=2.0, strength=0.25)
        two = g.glare(a * f32(2.0), 1, levels=levels, spread=2.0, strength=0.25)
        assert np.array_equal(two[..., :3], one[..., :3] * f32(2.0))
