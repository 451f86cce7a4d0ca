"""The display stage (EXTENSION) on the GPU against tests/display_ref.py: the histogram count for count, the
exposure within the ulps of one float64 log2, the adaptation recurrence, and the shown pixels bit for bit -- CLIP at ev = 0 is
Buffer.preview(), the other operators are the oracle's preview of the restated tone curve.  Frames are uploaded, not rendered,
except where a test says so."""
import os

import numpy as np
import pytest

import display_ref as ref
from conftest import GOLDEN
from helpers import gpu_scene

pytestmark = pytest.mark.gpu
f32 = np.float32

GOLDEN_FRAMES = ["scene_64x36_s4", "cornell2_48x48_s4", "volume_60x40_s4", "cloud_60x40_s4"]
SIZES = [(1, 1), (16, 17), (45, 35), (257, 3), (300, 200)]           # (width, height); the last: several strides per workgroup
LO, HI = f32(2.0 ** -16), f32(2.0 ** 16)


def upload(bendy, frame, samples=1, color_space=None):
    import torch
    frame = np.ascontiguousarray(frame, dtype=f32)
    buf = bendy.Buffer.new(frame.shape[1], frame.shape[0], bendy.ColorSpace.SRgb if color_space is None else color_space)
    buf.data.copy_(torch.from_numpy(frame))
    buf.samples = samples
    return buf


def edge_pixels():
    """Pixels on and next to the ends of the metered range, and the values no bin takes."""
    px = [np.array(v, dtype=f32) for v in ([0, 0, 0, 1], [-1, -1, -1, 1], [np.nan, 0.5, 0.5, 1], [np.inf, 0, 0, 1])]
    px += [ref.pixel_with_luminance(y) for y in (np.nextafter(LO, f32(0)), LO, np.nextafter(HI, f32(0)), HI)]
    return px


def lognormal_frame(w, h, seed):
    """Luminances spread over 2^-20 .. 2^20 (so some fall off either end), colours that are not grey."""
    rng = np.random.default_rng(seed)
    y = np.exp2(np.clip(rng.normal(0.0, 7.0, size=(h, w, 1)), -20, 20))
    a = (y * rng.uniform(0.2, 1.8, size=(h, w, 4))).astype(f32)
    a[..., 3] = 1.0
    return a


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))["iterative"]


def check_histogram(d, buf, frame, samples):
    d.present(buf)
    bins, under, over = d.histogram()
    want = ref.meter(frame, samples)
    assert np.array_equal(bins, want[0]) and (under, over) == want[1:], (np.flatnonzero(bins != want[0]), under, over, want[1:])
    assert int(bins.sum(dtype=np.uint64)) + under + over == frame.shape[0] * frame.shape[1]
    return bins


@pytest.mark.parametrize("w,h", SIZES)
def test_histogram_of_lognormal_frames_with_planted_edges(bendy, w, h):
    d = bendy.Display()
    frame = lognormal_frame(w, h, seed=w * 1000 + h)
    flat = frame.reshape(-1, 4)
    where = sorted({0, min(256, w * h - 1), w * h - 1})
    edges = edge_pixels()
    for turn in range(len(edges)):                      # every edge value visits every planted position
        for j, at in enumerate(where):
            flat[at] = edges[(turn + j) % len(edges)]
        for samples in ((1,) if turn else (1, 3, 4)):
            bins = check_histogram(d, upload(bendy, frame, samples), frame, samples)
    if w * h > 10000:
        assert np.count_nonzero(bins) > 200 and d.histogram()[1] > 0 and d.histogram()[2] > 0


@pytest.mark.parametrize("name", GOLDEN_FRAMES)
def test_histogram_of_golden_frames(bendy, name):
    d = bendy.Display()
    frame = golden(name)
    for samples in (1, 3, 4):
        check_histogram(d, upload(bendy, frame, samples), frame, samples)


def test_histogram_constant_zero_and_no_residue(bendy):
    d = bendy.Display()
    const = np.full((200, 300, 4), 0.5, dtype=f32)                     # every pixel in one bin: the worst case for the LDS adds
    bins = check_histogram(d, upload(bendy, const), const, 1)
    assert np.count_nonzero(bins) == 1 and bins.max() == 300 * 200
    zero = np.zeros((200, 300, 4), dtype=f32)
    bins = check_histogram(d, upload(bendy, zero), zero, 1)             # ... of which the next call shows no residue
    assert not bins.any() and d.histogram()[1:] == (300 * 200, 0)
    other = lognormal_frame(45, 35, seed=9)
    check_histogram(d, upload(bendy, other), other, 1)                  # another size on the same handle
    check_histogram(d, upload(bendy, const), const, 1)


def gpu_target(d, p):
    """The restatement's exposure for the histogram the GPU counted."""
    return ref.target(d.histogram()[0], {**ref.DEFAULTS, **p})


def ulps(a, b, scale=None):
    return abs(float(a) - float(b)) / float(np.spacing(f32(abs(scale if scale is not None else b))))


@pytest.mark.parametrize("name", GOLDEN_FRAMES)
def test_exposure_matches_the_restatement(bendy, name):
    d = bendy.Display()
    buf = upload(bendy, golden(name), 4)
    for p in (dict(), dict(ev=0.75, key=0.09, p_low=0.0, p_high=0.0), dict(p_low=0.45, p_high=0.45, ev=-1.25)):
        d.present(buf, **p)
        ev, mult = d.exposure()
        want = gpu_target(d, p)
        print(name, p, "ev", ev, "want", want, "mult", mult)
        assert ulps(ev, want) <= 2                                       # one float64 log2 on the host is the only inexact step
        assert abs(mult / 2.0 ** ev - 1.0) <= 1e-6
    # the known answers of tests/test_display_ref.py, through the GPU's own histogram
    d.present(buf)
    assert ulps(d.exposure()[0], ref.target(ref.meter(golden(name), 4)[0], ref.DEFAULTS)) <= 2


def test_exposure_clamps(bendy):
    d = bendy.Display()
    buf = upload(bendy, golden("scene_64x36_s4"), 4)
    d.present(buf)
    free = d.exposure()[0]
    for lo, hi, want in ((free + 1.0, 8.0, free + 1.0), (-8.0, free - 1.0, free - 1.0), (2.5, 2.5, 2.5)):
        d.present(buf, ev_min=lo, ev_max=hi)
        ev, mult = d.exposure()
        assert ev == f32(want) and abs(mult / 2.0 ** ev - 1.0) <= 1e-6


def test_adaptation_sequence_reset_black_frame_and_manual(bendy):
    A, B = upload(bendy, golden("scene_64x36_s4"), 4), upload(bendy, golden("cornell2_48x48_s4") * f32(9.0), 4)
    black = upload(bendy, np.zeros((8, 8, 4), dtype=f32))
    d = bendy.Display(adapt=0.5)

    def step(buf, state, **p):
        d.present(buf, **p)
        t = gpu_target(d, p)
        state = ref.adapt_step(state, t, p.get("adapt", 0.5))
        return state, t

    for attempt in range(2):                               # the same again after a reset
        state, ts = (f32(0), False), []
        for buf in (A, B, B):
            state, t = step(buf, state)
            ts.append(t)
            ev, mult = d.exposure()
            print("sequence", attempt, "ev", ev, "want", state[0], "target", t)
            # each target carries the float64 log2's ulp; the recurrence is a convex combination of the targets
            assert ulps(ev, state[0], scale=max(abs(v) for v in ts)) <= 2 and abs(mult / 2.0 ** ev - 1.0) <= 1e-6
        assert abs(float(ts[0]) - float(ts[1])) > 1.0 and state[0] != ts[1]       # the sequence does adapt
        before = d.exposure()
        # a black frame leaves the state alone and is shown with it
        d.present(black)
        assert d.histogram()[1:] == (64, 0) and d.exposure() == before
        # a manual call shows with its own ev and touches neither the state nor the last metered counters
        d.present(A, auto_exposure=0, ev=-1.5)
        assert d.exposure()[0] == -1.5 and abs(d.exposure()[1] / 2.0 ** -1.5 - 1.0) <= 1e-6 and d.histogram()[1:] == (64, 0)
        state2, t = step(A, state)
        assert ulps(d.exposure()[0], state2[0], scale=max(abs(v) for v in ts + [t])) <= 2
        d.reset()
        with pytest.raises(bendy.BendyError):
            d.exposure()
    # no state yet: a black frame is shown with params.ev, and the next metered frame still sets the exposure outright
    d.present(black, ev=0.5)
    assert d.exposure()[0] == 0.5
    d.present(B)
    assert ulps(d.exposure()[0], gpu_target(d, {})) <= 2
    # adapt = 1 has no memory
    d.present(A, adapt=1.0)
    assert ulps(d.exposure()[0], gpu_target(d, {})) <= 2


@pytest.fixture(scope="module")
def rendered(bendy):
    """scene and cornell2 at 45x35 x 4 samples: (Buffer, its host copy, the scene handle, the camera)."""
    import torch
    out = {}
    for name in ("scene", "cornell2"):
        sc, cam = gpu_scene(bendy, name, 45, 35)
        buf = bendy.Buffer.new(45, 35)
        bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4)).render(sc, cam, bendy.RenderConfig.with_samples(4), buf, seed=0x5EED)
        torch.cuda.synchronize()
        out[name] = (buf, buf.numpy().copy(), sc, cam)
    return out


@pytest.mark.parametrize("name", ["scene", "cornell2"])
def test_clip_at_ev0_is_the_preview(bendy, oracle, rendered, name):
    buf, host, _, _ = rendered[name]
    d = bendy.Display(tonemap="clip", auto_exposure=0, ev=0.0)
    try:
        for cs in (bendy.ColorSpace.SRgb, bendy.ColorSpace.Linear, bendy.ColorSpace.NONE):
            buf.color_space = cs
            got = d.present(buf)
            assert d.exposure() == (0.0, 1.0)
            assert np.array_equal(got, buf.preview()) and np.array_equal(got, oracle.preview(host, buf.samples, int(cs)))
    finally:
        buf.color_space = bendy.ColorSpace.SRgb


def special_frame():
    """NaN, negative, +inf and huge channels next to ordinary ones, alpha outside [0, 1] too."""
    a = lognormal_frame(16, 17, seed=4)
    a[0, 0] = (np.nan, 0.5, 2.0, 1.0)
    a[0, 1] = (-1.0, -0.0, 0.25, 0.5)
    a[0, 2] = (np.inf, 1.0, 0.0, 2.0)
    a[0, 3] = (3e38, 1e-38, 1.0, -1.0)
    a[0, 4] = (-np.inf, np.nan, np.inf, np.nan)
    return a


@pytest.mark.parametrize("op,white", [("reinhard", 1.0), ("reinhard", 4.0), ("aces", 4.0), ("clip", 4.0)])
def test_operators_bit_for_bit(bendy, oracle, rendered, op, white):
    d = bendy.Display(tonemap=op, white=white)
    code = {"clip": ref.CLIP, "reinhard": ref.REINHARD, "aces": ref.ACES}[op]
    frames = [(rendered[n][0], rendered[n][1]) for n in ("scene", "cornell2")]
    sp = special_frame()
    frames.append((upload(bendy, sp, 3), sp))
    try:
        for buf, host in frames:
            for cs in (bendy.ColorSpace.SRgb, bendy.ColorSpace.Linear):
                buf.color_space = cs
                for p in (dict(auto_exposure=0, ev=-2.0), dict(auto_exposure=0, ev=0.0), dict(auto_exposure=0, ev=1.5), dict()):
                    got = d.present(buf, **p)
                    ev, mult = d.exposure()
                    if "ev" in p:
                        assert ev == p["ev"]
                    assert abs(mult / 2.0 ** ev - 1.0) <= 1e-6
                    want = oracle.preview(ref.shown_frame(host, buf.samples, mult, code, white), 1, int(cs))
                    assert np.array_equal(got, want), (op, white, cs, p, np.argwhere(got != want)[:4])      # no pixel is exempt
    finally:
        for buf, _ in frames:
            buf.color_space = bendy.ColorSpace.SRgb


def test_special_values_map_as_defined(bendy):
    sp = special_frame()
    buf = upload(bendy, sp, 1, bendy.ColorSpace.Linear)
    got = bendy.Display(tonemap="aces", auto_exposure=0, ev=0.0).present(buf)
    assert list(got[0, 0][:1]) == [0] and list(got[0, 1][:2]) == [0, 0]           # NaN and negatives -> 0
    assert got[0, 2][0] == 0                                                       # ACES(inf) = inf / inf = NaN -> 0
    assert list(got[0, :5, 3]) == [255, 127, 255, 0, 0]                            # alpha: saturating, NaN -> 0
    clip = bendy.Display(tonemap="clip", auto_exposure=0, ev=0.0).present(buf)
    assert clip[0, 2][0] == 255 and clip[0, 0][0] == 0 and clip[0, 4][0] == 0      # CLIP: +inf saturates, NaN / -inf -> 0
    d = bendy.Display()
    d.present(buf)
    assert d.histogram()[1] >= 2 and d.histogram()[2] >= 1                          # they are metered as under / over


def test_nothing_else_moved(bendy, rendered):
    """Renders and previews on a scene handle before and after display calls (own handle, same stream) are identical."""
    import torch
    _, _, sc, cam = rendered["scene"]
    tr, rc = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4)), bendy.RenderConfig(samples=2, subsample=bendy.Subsample(2))

    def everything():
        plain = bendy.Buffer.new(45, 35)
        tr.render(sc, cam, rc, plain, seed=7)
        guided = [bendy.Buffer.new(45, 35) for _ in range(4)]
        tr.render_guided(sc, cam, rc, *guided, seed=7)
        ad = bendy.Adaptive(45, 35, threshold=0.05, min_samples=8, max_samples=16)
        abuf = bendy.Buffer.new(45, 35)
        for _ in range(3):
            tr.render_adaptive(sc, cam, rc, abuf, ad, seed=7)
        torch.cuda.synchronize()
        return [plain.numpy().copy(), plain.preview()] + [g.numpy().copy() for g in guided] + [abuf.numpy().copy(), ad.counts().copy()], plain

    before, buf = everything()
    d = bendy.Display(adapt=0.5)
    for p in (dict(), dict(tonemap="reinhard"), dict(tonemap="clip", auto_exposure=0, ev=1.0)):
        d.present(buf, **p)
    after, _ = everything()
    assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(buf.preview(), before[1]) and np.array_equal(buf.numpy(), before[0])     # present writes neither
