"""The glare stage's own per-texel code (csrc/bt_glare.hpp through bt_debug_glare_host; EXTENSION) against the
numpy restatement, bit for bit, on a machine without a GPU.  The kernels of bt_glare.hip call the same functions."""
import os

import numpy as np
import pytest

import glare_ref as g
from conftest import GOLDEN

f32 = np.float32
SHAPES = [(1, 1), (2, 1), (1, 2), (3, 5), (16, 17), (45, 35), (257, 3), (300, 200)]          # width x height
LEVELS, SAMPLES, SPREADS = (0, 1, 2, 3, 16), (1, 3, 4), (0.5, 1.0, 2.0)
GOLDEN_FRAMES = ["scene_64x36_s4", "cornell2_48x48_s4", "volume_60x40_s4", "cloud_60x40_s4"]


def settings():
    """levels x samples x spread in full; the strength takes turns."""
    return [(levels, samples, spread, (0.08, 0.5, 1.0)[(i + j + k) % 3]) for i, levels in enumerate(LEVELS)
            for j, samples in enumerate(SAMPLES) for k, spread in enumerate(SPREADS)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_host_entry_point_is_the_restatement(bendy, w, h):
    frame = g.make_frame(w, h, seed=w * 1000 + h)
    assert w * h < 4 or not np.isfinite(frame[..., :3]).all()
    for levels, samples, spread, strength in settings():
        got = bendy.glare_host(frame, samples, levels=levels, spread=spread, strength=strength)
        want = g.glare(frame, samples, levels=levels, spread=spread, strength=strength)
        assert np.isfinite(got[..., :3]).all()
        assert np.array_equal(got, want), (levels, samples, spread, strength, np.argwhere(got != want)[:4])      # no pixel is exempt


@pytest.mark.parametrize("name", GOLDEN_FRAMES)
def test_host_entry_point_on_golden_frames(bendy, name):
    frame = np.load(os.path.join(GOLDEN, name + ".npz"))["iterative"]
    for levels, samples, spread, strength in settings():
        got = bendy.glare_host(frame, samples, levels=levels, spread=spread, strength=strength)
        want = g.glare(frame, samples, levels=levels, spread=spread, strength=strength)
        assert np.array_equal(got, want), (levels, samples, spread, strength, np.argwhere(got != want)[:4])
    assert np.array_equal(bendy.glare_host(frame, 4), g.glare(frame, 4, **g.DEFAULTS))                 # the defaults
    assert np.array_equal(bendy.glare_host(frame, 4, max_value=0.5), g.glare(frame, 4, **{**g.DEFAULTS, "max_value": 0.5}))


def test_host_entry_point_validates(bendy):
    frame = g.make_frame(4, 4, poison=False)
    for bad in (dict(levels=17), dict(spread=0.0), dict(spread=17.0), dict(strength=1.5), dict(strength=float("nan")), dict(max_value=0.0),
                dict(max_value=float("inf"))):
        with pytest.raises(bendy.BendyError) as e:
            bendy.glare_host(frame, 1, **bad)
        assert e.value.code == -1, bad
    with pytest.raises(bendy.BendyError):
        bendy.glare_host(frame, 0)
    with pytest.raises(bendy.BendyError):
        bendy.glare_host(frame[..., :3], 1)
