"""The numpy restatement of the resample stage (tests/resample_ref.py; EXTENSION) held to the properties that follow
from its definition, without the library and without a GPU: identity, box at 2 : 1, constants, the tables' row sums and mirror
symmetry, what step 1 keeps out, the undershoot that step 5 removes, alpha, and linearity under a power of two."""
import numpy as np
import pytest

import resample_ref as r

f32 = np.float32
FILTERS = (r.BOX, r.TENT, r.MITCHELL, r.LANCZOS3)
# (w, h) -> (W, H): tests/test_resample_host.py's shapes
SHAPES = [((1, 1), (1, 1)), ((1, 1), (5, 3)), ((5, 3), (1, 1)), ((3, 5), (7, 2)), ((16, 17), (45, 35)), ((45, 35), (16, 17)),
          ((45, 35), (45, 35)), ((257, 3), (64, 3)), ((64, 36), (128, 72)), ((300, 200), (77, 51))]


@pytest.mark.parametrize("filt", (r.TENT, r.LANCZOS3))
def test_identity_is_the_sanitised_mean_bit_for_bit(filt):
    for w, h in ((1, 1), (3, 5), (45, 35), (257, 3)):
        first, T, wt, near = r.axis_table(w, w, filt)
        assert T == 2 * int(r.RADIUS[filt]) + 1
        assert np.array_equal(np.sort(wt, axis=1)[:, -1], np.ones(w, dtype=f32)) and np.count_nonzero(wt) == w      # {1.0} and zeros
        assert np.array_equal(near, np.arange(w))
        frame = r.make_frame(w, h, seed=w + h)
        for n in (1, 3):
            got = r.resample(frame, n, w, h, filter=filt)
            want = r.sanitise(frame, n, 65536.0)
            want[..., 3] = frame[..., 3]
            assert np.array_equal(got, want)


def test_box_at_two_to_one_is_a_half_and_a_half():
    for W in (1, 2, 8, 33):
        first, T, wt, near = r.axis_table(2 * W, W, r.BOX)
        assert T == 2 and np.array_equal(wt, np.full((W, 2), 0.5, dtype=f32)) and np.array_equal(first, 2 * np.arange(W))
        assert np.array_equal(near, 2 * np.arange(W) + 1)
    a = np.zeros((2, 4, 4), dtype=f32)
    a[..., 0] = [[1, 3, 5, 7], [9, 11, 13, 15]]
    a[..., 3] = 1.0
    assert np.array_equal(r.resample(a, 1, 2, 1, filter=r.BOX)[..., 0], [[6.0, 10.0]])


@pytest.mark.parametrize("src,dst", SHAPES)
def test_constants_come_back(src, dst):
    """A constant frame comes back within T_x + T_y ulps -- a product and a sum per tap -- apart from the rounding of the
    normalised weights: a row's float32 weights sum to 1 + e, and e scales the constant.  3.25 / n leaves the partial sums of
    the lobed filters (up to about 1.2 times the constant) in one binade, so one ulp is one size throughout."""
    (w, h), (W, H) = src, dst
    for filt in FILTERS:
        tx, ty = r.axis_table(w, W, filt), r.axis_table(h, H, filt)
        e = sum(np.abs(t[2].astype(np.float64).sum(axis=1) - 1.0).max() for t in (tx, ty))
        for n in (1, 3):
            frame = np.full((h, w, 4), 3.25, dtype=f32)
            c = f32(3.25) * (f32(1.0) / f32(n))
            out = r.resample(frame, n, W, H, filter=filt, tables=(tx, ty))
            bound = (tx[1] + ty[1]) * float(np.spacing(c)) + 1.01 * e * float(c)
            worst = float(np.abs(out[..., :3].astype(np.float64) - float(c)).max())
            print(src, dst, filt, n, "worst %.3g of bound %.3g" % (worst, bound))
            assert worst <= bound, (filt, n, worst, bound)
            assert np.array_equal(out[..., 3], np.full((H, W), 3.25, dtype=f32))


@pytest.mark.parametrize("src,dst", [(a[0], b[0]) for a, b in SHAPES] + [(a[1], b[1]) for a, b in SHAPES] + [(2100, 100), (21, 1)])
def test_rows_sum_to_one_and_tables_are_well_formed(src, dst):
    for filt in FILTERS:
        first, T, wt, near = r.axis_table(src, dst, filt)
        assert wt.shape == (dst, T) and T <= r.MAX_TAPS
        assert (np.abs(wt.astype(np.float64).sum(axis=1) - 1.0) <= T * 2.0 ** -23).all()          # T float32 ulps of 1
        assert (np.diff(first) >= 0).all() and (np.diff(near) >= 0).all() and near.min() >= 0 and near.max() <= src - 1
        assert first.min() >= -(T + 1) and (first + T - 1).max() <= src + T
        if filt in (r.BOX, r.TENT):
            assert (wt >= 0).all()


@pytest.mark.parametrize("src,dst", [(45, 16), (16, 45), (35, 35), (257, 64), (64, 128), (300, 77), (5, 1), (3, 7)])
def test_tables_mirror(src, dst):
    """Output dst - 1 - i takes source src - 1 - j with the weight output i gives j.  c_i and its mirror image are rounded on
    their own, so the weights may differ in the last place: one float32 ulp of 1 is allowed.  The box is half open, [-0.5, 0.5),
    so it mirrors only where no tap falls on its edge: it is held to this at whole ratios."""
    for filt in FILTERS:
        if filt == r.BOX and src % dst:
            continue
        first, T, wt, _ = r.axis_table(src, dst, filt)
        pad = T + 2
        dense = np.zeros((dst, src + 2 * pad), dtype=np.float64)
        for i in range(dst):
            dense[i, first[i] + pad:first[i] + pad + T] += wt[i]
        assert np.abs(dense - dense[::-1, ::-1]).max() <= 2.0 ** -23, filt


def test_poison_stays_out_and_does_not_spread():
    for (w, h), (W, H) in SHAPES:
        frame = r.make_frame(w, h, seed=7)
        clean = r.make_frame(w, h, seed=7, poison=False)
        assert w * h < 4 or not np.isfinite(frame[..., :3]).all()
        for filt in FILTERS:
            out = r.resample(frame, 1, W, H, filter=filt)
            assert np.isfinite(out).all() and (out[..., :3] >= 0).all() and (out[..., :3] <= 1.5 * 65536.0).all()
        # far from the poisoned pixels the output is that of the clean frame: a NaN reaches its own footprint only
        if (w, h, W, H) == (300, 200, 77, 51):
            a, b = r.resample(frame, 1, W, H, filter=r.LANCZOS3), r.resample(clean, 1, W, H, filter=r.LANCZOS3)
            assert np.array_equal(a[10:40], b[10:40]) and not np.array_equal(a, b)


def test_clamp_negative_removes_the_undershoot():
    frame = np.zeros((9, 9, 4), dtype=f32)
    frame[..., 3] = 1.0
    frame[4, 4, :3] = 100.0
    for W, H in ((27, 27), (9, 9), (13, 7)):
        raw = r.resample(frame, 1, W, H, filter=r.LANCZOS3, clamp_negative=0)
        cut = r.resample(frame, 1, W, H, filter=r.LANCZOS3, clamp_negative=1)
        if (W, H) == (9, 9):                                        # the identity has no lobes to undershoot with
            assert raw[..., :3].min() == 0 and np.array_equal(raw, cut)
            continue
        assert raw[..., :3].min() < -1.0 and cut[..., :3].min() == 0
        assert np.array_equal(cut[..., :3], np.maximum(raw[..., :3], 0))
    raw = r.resample(frame, 1, 27, 27, filter=r.MITCHELL, clamp_negative=0)
    assert raw[..., :3].min() < 0 and r.resample(frame, 1, 27, 27, filter=r.TENT, clamp_negative=0)[..., :3].min() == 0


def test_alpha_is_the_nearest_input_alpha():
    for (w, h), (W, H) in SHAPES:
        frame = r.make_frame(w, h, seed=3)
        ones = frame.copy()
        ones[..., 3] = 1.0
        for filt in FILTERS:
            for n in (1, 3):
                assert np.array_equal(r.resample(ones, n, W, H, filter=filt)[..., 3], np.ones((H, W), dtype=f32))
            got = r.resample(frame, 3, W, H, filter=filt)[..., 3]
            ys = np.minimum(h - 1, np.floor((np.arange(H) + 0.5) * (h / H))).astype(int)
            xs = np.minimum(w - 1, np.floor((np.arange(W) + 0.5) * (w / W))).astype(int)
            assert np.array_equal(got, frame[ys[:, None], xs[None, :], 3])


def test_twice_the_frame_is_twice_the_output():
    """Below the cap and above the subnormals every step commutes with a power of two."""
    for (w, h), (W, H) in SHAPES:
        frame = r.make_frame(w, h, seed=11, poison=False)
        frame[..., :3] *= f32(2.0 ** -6)                            # <= 2^14: twice it stays under 65536
        for filt in FILTERS:
            for n in (1, 3):
                one = r.resample(frame, n, W, H, filter=filt, clamp_negative=0)
                two_in = frame.copy()
                two_in[..., :3] *= f32(2.0)
                two = r.resample(two_in, n, W, H, filter=filt, clamp_negative=0)
                assert np.array_equal(two[..., :3], one[..., :3] * f32(2.0)) and np.array_equal(two[..., 3], one[..., 3])
