"""Properties of the despeckle stage's numpy restatement (tests/despeckle_ref.py; EXTENSION), on a machine without
a GPU: a smooth frame comes back untouched, the known answer for isolated pixels, pairs, blocks, lines and an L at every
setting the definition speaks of, the sanitiser, the scaling laws, and the counts on the committed 4-sample frames."""
import os

import numpy as np
import pytest

import despeckle_ref as d
from conftest import GOLDEN

f32 = np.float32
SHAPES = [(1, 1), (2, 1), (1, 2), (3, 5), (16, 17), (45, 35), (257, 3), (24, 32)]          # width x height
KNOWN = (32, 24)          # the known answer's frame: 32 wide, 24 high, so that (31, 23) is its last pixel

ISOLATED = [(10, 10), (0, 0), (31, 23), (15, 0), (0, 12)]
PAIR = [(20, 5), (21, 5)]
BLOCK = [(5, 18), (6, 18), (5, 19), (6, 19)]
LINE = [(x, 20) for x in range(12, 17)]
ELL = [(25, 15), (26, 15), (26, 16)]
# (radius, rank) -> the flagged pixels, as (x, y)
FLAGGED = {
    (1, 1): ISOLATED,
    (1, 2): ISOLATED + PAIR + [(12, 20), (16, 20)],
    (1, 3): ISOLATED + PAIR + LINE + ELL,
    (1, 4): ISOLATED + PAIR + BLOCK + LINE + ELL,
    (2, 2): ISOLATED + PAIR,
}


def known_frame():
    frame = d.ramp(*KNOWN)
    for x, y in ISOLATED + PAIR + BLOCK + LINE + ELL:
        frame[y, x, :3] = f32(1000.0)
    return frame


@pytest.mark.parametrize("w,h", SHAPES + [KNOWN])
def test_a_smooth_frame_comes_back(w, h):
    frame = d.ramp(w, h)
    for radius in (1, 2):
        out, det = d.despeckle(frame, 1, **{**d.DEFAULTS, "radius": radius}, details=True)
        assert np.array_equal(out, frame) and out.dtype == f32
        assert det["counts"] == (0, 0, w * h)


@pytest.mark.parametrize("radius,rank", sorted(FLAGGED))
def test_known_answer(radius, rank):
    frame = known_frame()
    out, det = d.despeckle(frame, 1, radius=radius, rank=rank, ratio=4.0, floor=0.0, details=True)
    got = sorted((int(x), int(y)) for y, x in np.argwhere(det["flagged"]))
    assert got == sorted(FLAGGED[(radius, rank)])
    # the changed pixels are exactly the flagged ones
    assert np.array_equal((out != frame).any(axis=-1), det["flagged"])
    assert np.array_equal(out[..., 3], frame[..., 3])
    # a flagged pixel's luminance is lim within the roundings on a term's path: three in Y (product, sum, sum), one in g = lim / Y,
    # one in s * g and three in the new luminance -- eight of at most 2^-24 relative each, and spacing(lim) > 2^-24 lim
    Y = d.luminance(out[..., :3])
    lim = det["lim"][det["flagged"]]
    assert (lim > 0).all() and (np.abs(Y[det["flagged"]] - lim) <= 8.0 * np.spacing(lim)).all()
    assert det["counts"][0] == len(FLAGGED[(radius, rank)]) and det["counts"][1] == 0


def test_sanitiser_and_its_count():
    frame = d.ramp(45, 35)
    bad = [f32(np.nan), f32(-3.0), f32(-np.inf), f32(np.inf), f32(3e38)]
    at = [(0, 0), (34, 44), (5, 7), (20, 20), (20, 21)]          # (y, x): the first, the last and three others
    for n, (y, x) in enumerate(at):
        frame[y, x, n % 3] = bad[n]
    frame[9, 9, :3] = f32(-0.0)                                    # passes unchanged: not counted
    frame[30, 3, 1] = f32(65536.0)                                 # the cap itself: not counted
    for radius, rank in ((1, 2), (2, 2), (2, 24)):
        out, det = d.despeckle(frame, 1, **{**d.DEFAULTS, "radius": radius, "rank": rank}, details=True)
        assert np.isfinite(out).all()
        assert det["counts"][1] == len(at)
        assert sorted(map(tuple, np.argwhere(det["sanitised"]))) == sorted(at)
        assert (out[..., :3] >= 0).all() and (out[..., :3] <= f32(65536.0)).all()
        assert np.signbit(out[9, 9, :3]).all()                     # -0.0 came back bit for bit
    # every channel of one pixel poisoned: still one sanitised pixel
    frame[1, 1, :3] = bad[:3]
    assert d.counts(frame, 1)[1] == len(at) + 1
    # with n samples the cap is max_value * n
    big = d.ramp(8, 8) * f32(100.0)
    out = d.despeckle(big, 4, **{**d.DEFAULTS, "max_value": 10.0})
    assert float(out[..., :3].max()) <= 40.0 and d.counts(big, 4, max_value=10.0)[1] == 64


def _speckled(seed=3, w=45, h=35):
    rng = np.random.default_rng(seed)
    frame = d.ramp(w, h)
    frame[..., :3] *= rng.uniform(0.5, 1.5, size=(h, w, 3)).astype(f32)
    for _ in range(12):
        frame[rng.integers(h), rng.integers(w), :3] *= f32(rng.uniform(20.0, 500.0))
    return frame


@pytest.mark.parametrize("radius,rank", [(1, 1), (1, 2), (1, 8), (2, 2), (2, 24)])
def test_scaling_laws(radius, rank):
    frame = _speckled()
    p = dict(radius=radius, rank=rank, ratio=4.0, floor=0.0, max_value=65536.0)
    one, det1 = d.despeckle(frame, 1, details=True, **p)
    assert 0 < det1["counts"][0] < frame.shape[0] * frame.shape[1]
    # a power of two commutes with every rounding: despeckle(2 frame) == 2 despeckle(frame), bit for bit, below the cap
    two, det2 = d.despeckle(frame * f32(2.0), 1, details=True, **p)
    assert np.array_equal(two[..., :3], one[..., :3] * f32(2.0)) and np.array_equal(det1["flagged"], det2["flagged"])
    # sums of four samples flag what their mean flags, the floor included: fl = floor * n
    p["floor"] = 0.01
    mean = d.despeckle(frame, 1, details=True, **p)[1]
    sums = d.despeckle(frame * f32(4.0), 4, details=True, **p)[1]
    assert np.array_equal(mean["flagged"], sums["flagged"]) and mean["counts"][0] > 0


def test_absent_taps_are_not_clamped():
    """A bright corner has three neighbours, all dim: it is flagged.  Replicated borders would make it its own neighbour."""
    frame = d.ramp(5, 4)
    frame[0, 0, :3] = frame[3, 4, :3] = f32(1000.0)
    for radius in (1, 2):
        det = d.despeckle(frame, 1, **{**d.DEFAULTS, "radius": radius}, details=True)[1]
        assert sorted(map(tuple, np.argwhere(det["flagged"]))) == [(0, 0), (3, 4)]
    assert np.array_equal(d.neighbour_count(5, 4, 1)[0], [3, 5, 5, 5, 3])
    assert d.neighbour_count(1, 1, 2)[0, 0] == 0 and d.neighbour_count(2, 1, 2)[0, 0] == 1 and d.neighbour_count(257, 3, 2)[1, 100] == 14
    # one pixel has no neighbour and is never flagged, however bright; of two, the brighter is judged against the other
    assert d.counts(np.full((1, 1, 4), 1e4, dtype=f32), 1)[0] == 0
    assert d.counts(np.array([[[1e4, 1e4, 1e4, 1], [1, 1, 1, 1]]], dtype=f32), 1, rank=8)[0] == 1


# flagged counts at n = 4 with the defaults
GOLDEN_COUNTS = {"cloud_60x40": 1, "cornell2_48x48": 14, "cornell_48x48": 16, "scene_64x36": 1, "volume_60x40": 1}


@pytest.mark.parametrize("name", sorted(GOLDEN_COUNTS))
def test_golden_frame_counts(name):
    frame = np.load(os.path.join(GOLDEN, name + "_s4.npz"))["iterative"]
    out, det = d.despeckle(frame, 4, **d.DEFAULTS, details=True)
    assert det["counts"][0] == GOLDEN_COUNTS[name]
    assert np.array_equal((out != frame).any(axis=-1), det["flagged"] | det["sanitised"])
    # nothing grows
    assert (out[..., :3] <= np.fmax(frame[..., :3], 0)).all()
