"""The despeckle stage's own per-pixel code (csrc/bt_despeckle.hpp through bt_debug_despeckle_host; EXTENSION)
against the numpy restatement, bit for bit and count for count, on a machine without a GPU.  The kernel of bt_despeckle.hip calls
the same functions."""
import os

import numpy as np
import pytest

import despeckle_ref as d
from conftest import GOLDEN
from glare_ref import make_frame

f32 = np.float32
SHAPES = [(1, 1), (2, 1), (1, 2), (3, 5), (16, 17), (45, 35), (257, 3), (24, 32)]          # width x height
SAMPLES, RATIOS = (1, 3, 4), (1.0, 4.0)
GOLDEN_FRAMES = ["scene_64x36_s4", "cornell2_48x48_s4", "cornell_48x48_s4", "volume_60x40_s4", "cloud_60x40_s4"]


def settings():
    """radius x rank x samples x ratio in full; rank N is the largest the radius takes."""
    return [(radius, rank, samples, ratio) for radius in (1, 2) for rank in (1, 2, d.max_rank(radius)) for samples in SAMPLES
            for ratio in RATIOS]


def selections():
    """One setting per selection the header has (two largest, four largest, counting) and per rank around their borders."""
    return [(radius, rank, 3, 2.0) for radius in (1, 2) for rank in (3, 4, 5, d.max_rank(radius) - 1)]


def check_host(bendy, frame, samples, **p):
    got, st = bendy.despeckle_host(frame, samples, stats=True, **p)
    want, det = d.despeckle(frame, samples, details=True, **{**d.DEFAULTS, **p})
    assert np.array_equal(got, want), (p, samples, np.argwhere(got != want)[:4])          # no pixel is exempt
    assert (st.flagged, st.sanitised, st.pixels) == det["counts"], (p, samples)
    return got, det


@pytest.mark.parametrize("w,h", SHAPES)
def test_host_entry_point_is_the_restatement(bendy, w, h):
    frame = make_frame(w, h, seed=w * 1000 + h)          # log-normal over 2^-20 .. 2^20; NaN, -3, +-inf, 3e38 at pixels 0, 256 and the last
    assert w * h < 4 or not np.isfinite(frame[..., :3]).all()
    flagged = 0
    for radius, rank, samples, ratio in settings():
        got, det = check_host(bendy, frame, samples, radius=radius, rank=rank, ratio=ratio)
        assert np.isfinite(got[..., :3]).all()
        flagged += det["counts"][0]
    for radius, rank, samples, ratio in selections():
        check_host(bendy, frame, samples, radius=radius, rank=rank, ratio=ratio)
    assert flagged > 0 or w * h == 1                       # the frames exercise both branches of step 6


@pytest.mark.parametrize("name", GOLDEN_FRAMES)
def test_host_entry_point_on_golden_frames(bendy, name):
    frame = np.load(os.path.join(GOLDEN, name + ".npz"))["iterative"]
    for radius, rank, samples, ratio in settings():
        check_host(bendy, frame, samples, radius=radius, rank=rank, ratio=ratio)
    for radius, rank, samples, ratio in selections():
        check_host(bendy, frame, samples, radius=radius, rank=rank, ratio=ratio)
    check_host(bendy, frame, 4)                            # the defaults
    check_host(bendy, frame, 4, max_value=0.5, floor=0.0)


def test_smooth_frames_and_minus_zero_come_back_bit_for_bit(bendy):
    for w, h in SHAPES:
        frame = d.ramp(w, h)
        if min(w, h) >= 3:                                 # where its neighbours still have two brighter ones each
            frame[0, 0, :3] = f32(-0.0)
        got, st = bendy.despeckle_host(frame, 1, stats=True)
        assert got.tobytes() == frame.tobytes() and (st.flagged, st.sanitised, st.pixels) == (0, 0, w * h)


def test_host_entry_point_validates(bendy):
    frame = make_frame(4, 4, poison=False)
    for bad in (dict(radius=0), dict(radius=3), dict(rank=0), dict(rank=9), dict(radius=2, rank=25), dict(ratio=0.5), dict(ratio=float("nan")),
                dict(floor=-1.0), dict(floor=float("inf")), dict(max_value=0.0), dict(max_value=float("inf"))):
        with pytest.raises(bendy.BendyError) as e:
            bendy.despeckle_host(frame, 1, **bad)
        assert e.value.code == -1, bad
    with pytest.raises(bendy.BendyError):
        bendy.despeckle_host(frame, 0)
    with pytest.raises(bendy.BendyError):
        bendy.despeckle_host(frame[..., :3], 1)
