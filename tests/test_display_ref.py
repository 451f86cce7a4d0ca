"""tests/display_ref.py, the numpy restatement of the display stage (EXTENSION), on its own: the exposures of the
golden frames as known answers, the edges of the luminance bins, the counters' sum, the black-frame rule and the adaptation
recurrence.  No GPU, no library."""
import os

import numpy as np
import pytest

import display_ref as ref
from conftest import GOLDEN

f32 = np.float32

# the restatement's `e` under bt_display_params_default, computed on the CPU from the definition in include/bendy_hip.h
KNOWN = {"scene_64x36_s4": (0.96233606, 0), "cornell2_48x48_s4": (0.50997084, 166), "volume_60x40_s4": (1.147963, 0),
         "cloud_60x40_s4": (1.1514534, 0)}


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))["iterative"]


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_exposures_of_the_golden_frames(name):
    frame = golden(name)
    bins, under, over = ref.meter(frame, 4)
    e, want_under = KNOWN[name]
    assert (under, over) == (want_under, 0)
    assert int(bins.sum()) + under + over == frame.shape[0] * frame.shape[1]
    t = ref.target(bins, ref.DEFAULTS)
    assert t.dtype == f32 and t == f32(e)
    assert ref.adapt_step((f32(0), False), t, 1.0) == (f32(e), True)
    assert abs(float(ref.exp2_bt(t)) / 2.0 ** float(t) - 1.0) <= 1e-6


def test_bin_edges():
    lo, hi = f32(2.0 ** -16), f32(2.0 ** 16)
    below_lo, below_hi = np.nextafter(lo, f32(0)), np.nextafter(hi, f32(0))
    cases = [(f32(0.0), "under"), (f32(-1.0), "under"), (f32(np.nan), "under"), (below_lo, "under"), (f32(-np.inf), "under"),
             (f32(np.inf), "over"), (hi, "over"), (lo, 0), (below_hi, 255), (f32(1.0), 128), (f32(1.12), 128), (f32(1.125), 129),
             (f32(0.18), 107)]           # bins split an octave linearly: 0.18 = 1.44 * 2^-3 -> (124 - 111) * 8 + 3
    for y, want in cases:
        px = np.array([[0, y, 0, 1]], dtype=f32) if not np.isfinite(y) or y <= 0 else ref.pixel_with_luminance(y)[None]
        bins, under, over = ref.meter(px, 1)
        if want == "under":
            assert (int(bins.sum()), under, over) == (0, 1, 0), y
        elif want == "over":
            assert (int(bins.sum()), under, over) == (0, 0, 1), y
        else:
            assert bins[want] == 1 and (int(bins.sum()), under, over) == (1, 0, 0), (y, np.flatnonzero(bins))
    # the sample count divides first: sums of 3 samples whose mean is 2^-16 land where the mean does
    px = ref.pixel_with_luminance(lo)[None] * f32(4.0)
    assert ref.meter(px, 4)[0][0] == 1 and ref.meter(px, 1)[0][16] == 1


def test_counters_sum_to_the_pixel_count():
    rng = np.random.default_rng(15)
    a = np.exp2(rng.uniform(-22, 22, size=(37, 29, 4))).astype(f32)
    a[0, 0, :3] = np.nan
    a[5, 7, :3] = -3.0
    a[36, 28, :3] = np.inf
    a[9, 9, :3] = 0.0
    for n in (1, 3, 4):
        bins, under, over = ref.meter(a, n)
        assert int(bins.sum()) + under + over == 37 * 29 and under >= 3 and over >= 1 and bins.sum() > 0


def test_percentiles_and_the_mean_of_the_bin_centres():
    h = np.zeros(256, dtype=np.uint32)
    h[100], h[120], h[200] = 10, 80, 10
    p = dict(ref.DEFAULTS, p_low=0.1, p_high=0.1, ev=0.0)
    # lo = 10, hi = 90: exactly the 80 pixels of bin 120 are left; its centre is (2 * 120 + 1) / 16 - 16 = -0.9375
    assert ref.target(h, p) == f32(np.log2(0.18) + 0.9375)
    assert ref.target(h, dict(p, ev=1.5)) == f32(np.log2(0.18) + 0.9375) + f32(1.5)
    # no trimming: the mean over all three bins, weighted by their counts
    m = (10 * 201 + 80 * 241 + 10 * 401) / (16.0 * 100) - 16.0
    assert ref.target(h, dict(p, p_low=0.0, p_high=0.0)) == f32(np.log2(0.18) - m)
    # clamping
    assert ref.target(h, dict(p, ev_min=3.0)) == f32(3.0) and ref.target(h, dict(p, ev_max=-3.0)) == f32(-3.0)


def test_black_frame_leaves_the_state_alone():
    z = np.zeros((4, 4, 4), dtype=f32)
    bins, under, over = ref.meter(z, 1)
    assert (int(bins.sum()), under, over) == (0, 16, 0)
    assert ref.target(bins, ref.DEFAULTS) is None
    for state in ((f32(0), False), (f32(1.25), True)):
        assert ref.adapt_step(state, None, 0.5) == state
    p = dict(ref.DEFAULTS, ev=-0.75)
    assert ref.shown_ev((f32(0), False), p) == f32(-0.75) and ref.shown_ev((f32(1.25), True), p) == f32(1.25)
    # p_low + p_high < 1 keeps at least one pixel of a frame that has any in range: W == 0 only when N == 0
    h = np.zeros(256, dtype=np.uint32)
    h[7] = 1
    assert ref.target(h, dict(ref.DEFAULTS, p_low=0.5, p_high=0.49)) == ref.target(h, dict(ref.DEFAULTS, p_low=0.0, p_high=0.0))


def test_adaptation_recurrence():
    a, b = f32(2.0), f32(-1.0)
    s = (f32(0), False)
    s = ref.adapt_step(s, a, 0.5)
    assert s == (a, True)                                  # the first frame sets the exposure outright
    s = ref.adapt_step(s, b, 0.5)
    assert s[0] == f32(0.5)
    s = ref.adapt_step(s, b, 0.5)
    assert s[0] == f32(-0.25)
    assert ref.adapt_step(s, a, 1.0)[0] == a               # adapt >= 1: no memory
    e, t, k = f32(0.3), f32(1.7), f32(0.3)
    assert ref.adapt_step((e, True), t, k)[0] == e + (t - e) * k


def test_operators():
    x = np.array([[-1.0, 0.0, np.nan], [0.5, 1.0, 4.0], [np.inf, 1e-3, 100.0]], dtype=f32)
    assert np.array_equal(ref.tone(x, 1.0, ref.CLIP), x, equal_nan=True)
    r = ref.tone(x, 1.0, ref.REINHARD, white=4.0)
    assert r.dtype == f32 and list(r[0]) == [0, 0, 0] and r[1, 2] == f32(1.0)          # the white point maps to 1
    assert r[1, 0] == (f32(0.5) * (f32(1) + f32(0.5) * (f32(1) / f32(16)))) / f32(1.5)
    a = ref.tone(x, 2.0, ref.ACES)
    assert list(a[0]) == [0, 0, 0] and a[1, 0] == (f32(1) * (f32(2.51) + f32(0.03))) / (f32(1) * (f32(2.43) + f32(0.59)) + f32(0.14))
    assert np.isnan(r[2, 0]) and np.isnan(a[2, 0])                                       # inf / inf
    f = ref.shown_frame(np.array([[[2.0, 4.0, 6.0, 0.5]]], dtype=f32), 2, 1.0, ref.CLIP)
    assert f.tolist() == [[[1.0, 2.0, 3.0, 0.5]]]
