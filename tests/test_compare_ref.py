"""tests/compare_ref.py -- the numpy restatement of the compare stage (EXTENSION) -- against the properties the
definition promises: the identity, symmetry of the MSE, agreement with the float64 relMSE formula the other tests use, the tail
on a single wrong pixel and on a plane of ties, the first of equal maxima, non-finite pixels, and the map's ramp.  No GPU, no
library."""
import math

import numpy as np
import pytest

import compare_ref as c

f32 = np.float32


@pytest.mark.parametrize("poison", [None, "nonfinite", "big"])
def test_identity(poison):
    X, _ = c.make_pair(45, 35, seed=1, poison=poison)
    r = c.measure(X, X)
    assert r["mse"] == 0.0 and r["rel_mse"] == 0.0 and r["max_abs"] == 0.0 and r["max_index"] == 0
    assert (r["s"] == 1.0).all()           # numerator and denominator are the same bits
    assert r["ssim"] == 1.0                # and a sum of ones is exact
    assert r["psnr"] == math.inf
    assert r["valid"] + r["nonfinite"] == r["pixels"] == 45 * 35
    assert r["nonfinite"] == (2 if poison == "nonfinite" else 0)       # the spots of X alone: 0 and 256
    for f in (0.01, 0.5, 1.0):
        assert c.tail(r["E"], f) == (0.0, 0.0)


def test_mse_is_symmetric_bit_for_bit():
    for seed, noise in ((2, 0.05), (3, 0.8)):
        X, Y = c.make_pair(33, 33, seed=seed, noise=noise, nx=3, ny=4)
        a, b = c.measure(X, Y, 3, 4), c.measure(Y, X, 4, 3)
        assert a["mse"] == b["mse"] and a["max_abs"] == b["max_abs"] and a["max_index"] == b["max_index"] and a["mse"] > 0


def test_rel_mse_agrees_with_the_formula_in_use():
    """All terms are non-negative, so any summation order of N float64 terms is within N 2^-53 of exact: N = 3 * 128 * 128 gives
    5.5e-12, inside rtol 1e-10."""
    rng = np.random.default_rng(4)
    y = np.ones((128, 128, 4), dtype=f32)
    y[..., :3] = np.exp2(rng.uniform(-6.0, 6.0, size=(128, 128, 3))).astype(f32)
    x = y.copy()
    x[..., :3] = (y[..., :3] * (1.0 + 0.3 * rng.standard_normal((128, 128, 3)))).astype(f32)
    got, want = c.measure(x, y)["rel_mse"], c.rel_mse_numpy(x, y)
    print("rel_mse", got, "formula", want, "relative difference", abs(got - want) / want)
    assert math.isclose(got, want, rel_tol=1e-10)


def test_one_wrong_pixel_carries_everything():
    Y = np.full((35, 45, 4), 0.5, dtype=f32)
    X = Y.copy()
    X[20, 17, 1] = 0.75
    r = c.measure(X, Y)
    assert r["max_index"] == 20 * 45 + 17 and r["max_abs"] == 0.25
    for f in (1e-6, 0.01, 0.5, 1.0):
        share, T, det = c.tail(r["E"], f, details=True)
        assert share == 1.0, f
        assert (T > 0) == (det["k"] == 1)


def test_ties_path():
    """A constant error plane: nothing is above the threshold, the share is k c / S_all."""
    Y = np.full((36, 64, 4), 0.5, dtype=f32)
    X = np.full((36, 64, 4), 0.625, dtype=f32)
    r = c.measure(X, Y)
    cst = r["E"][0, 0]
    assert cst > 0 and (r["E"] == cst).all()
    for f in (0.01, 0.25, 1.0):
        share, T, det = c.tail(r["E"], f, details=True)
        assert T == cst and det["c_gt"] == 0 and det["k"] == math.ceil(f * 36 * 64)
        assert share == float(np.float64(det["k"]) * np.float64(cst) / np.float64(det["S_all"]))


def test_first_of_equal_maxima():
    Y = np.zeros((17, 16, 4), dtype=f32)
    X = Y.copy()
    for p in (200, 37, 250):
        X.reshape(-1, 4)[p, p % 3] = 2.0
    r = c.measure(X, Y)
    assert r["max_abs"] == 2.0 and r["max_index"] == 37


def test_bad_pixels_are_counted_and_leave_the_sums_finite():
    X, Y = c.make_pair(33, 33, seed=5, poison="nonfinite")
    r = c.measure(X, Y)
    assert c.spots(33, 33) == [0, 256, 33 * 33 - 1]
    assert r["nonfinite"] == 3 and r["valid"] == 33 * 33 - 3
    assert all(math.isfinite(r[k]) for k in ("mse", "rel_mse", "ssim", "max_abs", "psnr"))
    E = r["E"].ravel()
    assert np.signbit(E[[0, 256, -1]]).all() and (E[[0, 256, -1]] == 0).all() and np.signbit(E).sum() == 3
    assert np.isfinite(r["s"]).all() and (r["v"].reshape(-1, 2)[[0, 256, -1]] == 0).all()
    share, T = c.tail(r["E"], 1.0)
    # S_gt and S_all add the same non-negative terms in two trees: each is within N 2^-53 of exact, N = 33 * 33
    assert math.isclose(share, 1.0, rel_tol=1e-12) and T >= 0


def test_map_ramp():
    E = np.array([[0.0, 1 / 3, 2 / 3, 1.0, 7.0, -0.0]], dtype=f32)
    got = c.error_map(E, 1.0)[0]
    third = int(f32(3.0) * f32(1 / 3) * f32(255.0) + f32(0.5))
    two = f32(3.0) * f32(2 / 3)
    assert got[0].tolist() == [0, 0, 0, 255]
    assert got[1].tolist() == [min(third, 255), int(max(f32(3.0) * f32(1 / 3) - f32(1.0), 0) * f32(255.0) + f32(0.5)), 0, 255]
    assert got[2].tolist() == [255, int(min(two - f32(1.0), f32(1.0)) * f32(255.0) + f32(0.5)), int(max(two - f32(2.0), 0) * f32(255.0) + f32(0.5)), 255]
    assert got[3].tolist() == [255, 255, 255, 255] and got[4].tolist() == [255, 255, 255, 255]
    assert got[5].tolist() == [255, 0, 255, 255]          # a bad pixel is magenta
    assert got[1][0] == 255 and got[1][1] <= 1 and got[2][1] >= 254 and got[2][2] <= 1
    assert c.error_map(E, 7.0)[0, 4].tolist() == [255, 255, 255, 255] and c.error_map(E, 14.0)[0, 4, 2] == 0
