"""The despeckle stage (EXTENSION) on the GPU against tests/despeckle_ref.py, bit for bit and count for count: the
output and the counters, frames that cross tile borders, a handle that serves frames of changing size, renders left alone, the
stage ahead of the glare stage, and what it does to the error of a 4-sample frame.  Frames are uploaded, not rendered, except
where a test says so."""
import os

import numpy as np
import pytest

import despeckle_ref as d
import glare_ref
from conftest import GOLDEN
from helpers import gpu_scene
from test_despeckle_host import GOLDEN_FRAMES, SHAPES, selections, settings

pytestmark = pytest.mark.gpu
f32 = np.float32
# one column or one row into a second tile; halos that cross tile corners
GPU_SHAPES = SHAPES + [(17, 16), (33, 33)]


def upload(bendy, frame, samples=1):
    import torch
    frame = np.ascontiguousarray(frame, dtype=f32)
    buf = bendy.Buffer.new(frame.shape[1], frame.shape[0])
    buf.data.copy_(torch.from_numpy(frame))
    buf.samples = samples
    return buf


def check_call(bendy, handle, frame, samples, **p):
    """One apply against the restatement: the output and the three counts."""
    out = handle.apply(upload(bendy, frame, samples), **p)
    assert out.samples == samples                                   # sums of the same count, not a mean
    got, st = out.numpy(), handle.poll()
    want, det = d.despeckle(frame, samples, details=True, **{**d.DEFAULTS, **p})
    assert np.array_equal(got, want), (p, samples, np.argwhere(got != want)[:4])          # no pixel is exempt
    assert (st.flagged, st.sanitised, st.pixels) == det["counts"], (p, samples)
    return got


@pytest.mark.parametrize("w,h", GPU_SHAPES)
def test_device_is_the_restatement(bendy, w, h):
    handle = bendy.Despeckle()
    frame = glare_ref.make_frame(w, h, seed=w * 1000 + h)
    for radius, rank, samples, ratio in settings() + selections():
        got = check_call(bendy, handle, frame, samples, radius=radius, rank=rank, ratio=ratio)
        assert np.isfinite(got[..., :3]).all()
    # a smooth frame comes back bit for bit, -0.0 included
    smooth = d.ramp(w, h)
    if min(w, h) >= 3:
        smooth[0, 0, :3] = f32(-0.0)
    assert check_call(bendy, handle, smooth, 1).tobytes() == smooth.tobytes()


@pytest.mark.parametrize("name", GOLDEN_FRAMES)
def test_device_on_golden_frames(bendy, name):
    handle = bendy.Despeckle()
    frame = np.load(os.path.join(GOLDEN, name + ".npz"))["iterative"]
    for radius, rank, samples, ratio in settings() + selections():
        check_call(bendy, handle, frame, samples, radius=radius, rank=rank, ratio=ratio)
    check_call(bendy, handle, frame, 4)                          # the defaults
    check_call(bendy, handle, frame, 4, max_value=0.5, floor=0.0)


def test_more_tile_rows_than_a_grid_axis_takes(bendy):
    """The grid of tiles is one-dimensional: a frame of 65 538 tile rows, beyond what grid.y takes, is no special case."""
    h = 65537 * 16 + 3
    rng = np.random.default_rng(5)
    frame = np.ones((h, 1, 4), dtype=f32)
    frame[..., :3] = np.exp2(rng.normal(0.0, 2.0, size=(h, 1, 3))).astype(f32)
    handle = bendy.Despeckle()
    check_call(bendy, handle, frame, 1, radius=2, rank=2)
    check_call(bendy, handle, frame, 1, radius=1, rank=2, ratio=1.0)


def test_handle_serves_frames_of_changing_size(bendy):
    P = dict(radius=2, rank=3, ratio=2.0)
    handle = bendy.Despeckle()
    mid, small, large = glare_ref.make_frame(45, 35, seed=1), glare_ref.make_frame(3, 5, seed=2), glare_ref.make_frame(300, 200, seed=3)
    first = check_call(bendy, handle, mid, 3, **P)
    check_call(bendy, handle, small, 1, **P)
    check_call(bendy, handle, large, 4, **P)
    check_call(bendy, handle, np.full((1, 1, 4), 2.5, dtype=f32), 1, **P)                   # M = 0: never flagged
    assert handle.poll().flagged == 0 and handle.poll().pixels == 1
    assert np.array_equal(check_call(bendy, handle, mid, 3, **P), first)
    assert np.array_equal(check_call(bendy, bendy.Despeckle(), mid, 3, **P), first)         # a fresh handle agrees
    handle = bendy.Despeckle(**P)                                                           # the handle's own parameters
    # out= is written in place; the input is left alone
    buf = upload(bendy, mid, 3)
    out = bendy.Buffer.new(45, 35)
    assert handle.apply(buf, out=out) is out and np.array_equal(out.numpy(), first) and np.array_equal(buf.numpy(), mid, equal_nan=True)
    assert out.samples == 3 and out.color_space == buf.color_space
    with pytest.raises(bendy.BendyError):
        handle.apply(buf, out=buf)


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
def test_renders_are_left_alone(bendy, rendered, name):
    """A render on the same scene handle, its preview and its display are bit-identical before and after apply calls."""
    import torch
    buf, host, sc, cam = rendered[name]
    tr, rc = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4)), bendy.RenderConfig.with_samples(4)

    def everything():
        again = bendy.Buffer.new(45, 35)
        tr.render(sc, cam, rc, again, seed=0x5EED)
        torch.cuda.synchronize()
        return [again.numpy().copy(), again.preview(), bendy.Display().present(again)]

    before = everything()
    assert np.array_equal(before[0], host)
    handle = bendy.Despeckle()
    for p in (dict(), dict(radius=2, rank=24, ratio=1.0), dict(rank=1, floor=0.0)):
        check_call(bendy, handle, host, 4, **p)
        handle.apply(buf, **p)
    after = everything()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(buf.numpy(), host)                     # apply does not write its input


@pytest.mark.parametrize("name", ["scene", "cornell2"])
def test_despeckle_then_glare(bendy, rendered, name):
    """Glare().apply(Despeckle().apply(buf)) is the glare's restatement applied to the despeckle's: the stage hands on sums and
    their count."""
    buf, host, _, _ = rendered[name]
    for p, q in ((dict(), dict()), (dict(radius=2, rank=3, ratio=2.0), dict(strength=0.5, levels=3, spread=2.0))):
        got = bendy.Glare().apply(bendy.Despeckle().apply(buf, **p), **q)
        want = glare_ref.glare(d.despeckle(host, buf.samples, **{**d.DEFAULTS, **p}), buf.samples, **{**glare_ref.DEFAULTS, **q})
        assert got.samples == 1 and np.array_equal(got.numpy(), want), (p, q)
    assert d.counts(host, buf.samples)[0] > 0                     # and there was something to pull down


# ---- it helps, or it does not -------------------------------------------------------------------------------------------------

def rel_mse(x, y):
    """mean((x - y)^2 / (y^2 + 0.01)), DESIGN.md 11."""
    x, y = x[..., :3].astype(np.float64), y[..., :3].astype(np.float64)
    return float(np.mean((x - y) ** 2 / (y ** 2 + 0.01)))


_frames = {}


def quality_frames(bendy, name, w=128, h=128):
    """4 x Subpixel(2) samples of colour and guides, and a truth of 1024 samples per pixel (256 x Subpixel(2)) from another seed."""
    import torch
    if (name, w, h) not in _frames:
        sc, cam = gpu_scene(bendy, name, w, h)
        tr = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4))
        bufs = [bendy.Buffer.new(w, h) for _ in range(4)]
        tr.render_guided(sc, cam, bendy.RenderConfig(samples=4, subsample=bendy.Subsample(2)), *bufs, seed=0x5EED)
        truth = bendy.Buffer.new(w, h)
        tr.render(sc, cam, bendy.RenderConfig(samples=256, subsample=bendy.Subsample(2)), truth, seed=0xBEEF)
        torch.cuda.synchronize()
        _frames[(name, w, h)] = (bufs, truth)
    return _frames[(name, w, h)]


def quality(bendy, name, params=None):
    """relMSE ratios against the truth: despeckled / raw and denoise(despeckled) / denoise(raw); and the cost to legitimate
    detail, measured on the truth frame itself: the share of its pixels the stage flags and relMSE(despeckle(truth), truth)."""
    (color, albedo, normal, depth), truth = quality_frames(bendy, name)
    handle = bendy.Despeckle(**(params or {}))
    y = truth.mean()
    clean = handle.apply(color)
    st = handle.poll()
    raw, desp = rel_mse(color.mean(), y), rel_mse(clean.mean(), y)
    den_raw = rel_mse(bendy.denoise(color, albedo, normal, depth).numpy(), y)
    den_desp = rel_mse(bendy.denoise(clean, albedo, normal, depth).numpy(), y)
    on_truth = handle.apply(truth)
    ts = handle.poll()
    return dict(plain=desp / raw, denoised=den_desp / den_raw, raw=raw, denoised_raw=den_raw, flagged=st.flagged / st.pixels,
                truth_flagged=ts.flagged / ts.pixels, truth_cost=rel_mse(on_truth.mean(), y))


# relMSE(despeckled) / relMSE(raw) and relMSE(denoise(despeckled)) / relMSE(denoise(raw)) with the default parameters, as measured
# on an MI355X, plus the 25 % DESIGN.md 11 and 14 give their ratios for seed-to-seed spread.  Only a scene whose
# measured ratio x 1.25 is below 1 has a bound; the others are printed.
HELPS_BOUNDS = {"scene": (0.919, None), "cornell2": (0.375, 0.836), "volume": (0.365, None)}
# measured: plain 0.7350 / 0.2997 / 0.2915, denoised pair 0.9222 / 0.6686 / 0.9873 on scene / cornell2 / volume


@pytest.mark.parametrize("name", ["scene", "cornell2", "volume"])
def test_it_helps_a_four_sample_frame(bendy, name):
    r = quality(bendy, name)
    print(f"{name}: relMSE ratio despeckled / raw {r['plain']:.4f}, denoised pair {r['denoised']:.4f} (raw relMSE {r['raw']:.5f}, "
          f"denoised raw {r['denoised_raw']:.5f}); flagged {r['flagged']:.5f} of the frame, {r['truth_flagged']:.5f} of the truth, "
          f"relMSE(despeckle(truth), truth) {r['truth_cost']:.3e}")
    b_plain, b_denoised = HELPS_BOUNDS[name]
    assert r["plain"] <= b_plain and r["plain"] < 1
    if b_denoised is not None:
        assert r["denoised"] <= b_denoised and r["denoised"] < 1
