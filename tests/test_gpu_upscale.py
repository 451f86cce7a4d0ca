"""The upscale stage (EXTENSION) on the GPU against tests/upscale_ref.py, bit for bit and count for count: the
output, the prepared planes and the counters, a frame of more tile rows than a grid axis takes, a handle that serves frames of
changing size, renders and the other stages left alone, the stage ahead of the glare stage, and what it does to the error of a
small render shown large.  Frames are uploaded, not rendered, except where a test says so."""
import numpy as np
import pytest

import glare_ref
import upscale_ref as u
from helpers import gpu_scene
from test_upscale_host import SHAPES, cases, frames

pytestmark = pytest.mark.gpu
f32 = np.float32


def upload(bendy, frame, samples=1):
    import torch
    frame = np.ascontiguousarray(frame, dtype=f32)
    buf = bendy.Buffer.new(frame.shape[1], frame.shape[0])
    buf.data.copy_(torch.from_numpy(frame))
    buf.samples = samples
    return buf


def upload_guides(bendy, guides):
    return tuple(None if g is None else upload(bendy, *g) for g in guides)


def check_call(bendy, handle, color, samples, lo, hi, W, H, **p):
    """One apply against the restatement: the output, the three prepared planes and the three counts."""
    out = handle.apply(upload(bendy, color, samples), W, H, lo=upload_guides(bendy, lo), hi=upload_guides(bendy, hi), **p)
    assert out.samples == 1 and (out.width, out.height) == (W, H)                     # a mean
    got, st = out.numpy(), handle.poll()
    q = {**u.DEFAULTS, **p}
    want, det = u.upscale(color, samples, W, H, lo=lo, hi=hi, details=True, **q)
    assert np.array_equal(got, want), (p, samples, np.argwhere(got != want)[:4])       # no pixel is exempt
    assert (st.tier2, st.tier3, st.pixels) == det["counts"], (p, samples)
    for which, plane in enumerate(u.planes(color, samples, lo, q["max_value"])):
        assert np.array_equal(handle.plane(which), plane), which
    return got


@pytest.mark.parametrize("w,h,W,H", SHAPES)
def test_device_is_the_restatement(bendy, w, h, W, H):
    handle = bendy.Upscale()
    for color, samples, lo, hi, p in cases(w, h, W, H):
        got = check_call(bendy, handle, color, samples, lo, hi, W, H, **p)
        assert np.isfinite(got[..., :3]).all()
    for axis, (src, dst) in enumerate(((w, W), (h, H))):
        first, weights, nearest = handle.weights(axis)
        rf, rw, rn = u.axis_table(src, dst)
        assert np.array_equal(first, rf) and np.array_equal(weights, rw) and np.array_equal(nearest, rn)


def test_equal_sizes_return_the_sanitised_mean(bendy):
    color = u.make_frame(45, 35, seed=9)
    g = u.make_guides(45, 35, seed=9, poison=False)
    pair = (g[0], None, g[2])
    handle = bendy.Upscale()
    got = check_call(bendy, handle, color, 3, pair, pair, 45, 35)
    assert np.array_equal(got[..., :3], u.sanitise(color, 3, 65536.0)[..., :3]) and handle.poll().tier2 == handle.poll().tier3 == 0


def test_more_tile_rows_than_a_grid_axis_takes(bendy):
    """The grid of tiles is one-dimensional: an output of 65 538 tile rows, beyond what grid.y takes, is no special case."""
    h, H = 65600, 65537 * 16 + 3
    rng = np.random.default_rng(5)
    color = np.ones((h, 1, 4), dtype=f32)
    color[..., :3] = np.exp2(rng.normal(0.0, 2.0, size=(h, 1, 3))).astype(f32)
    lo_z, hi_z = np.ones((h, 1, 4), dtype=f32), np.ones((H, 1, 4), dtype=f32)
    lo_z[..., 0] = 1.0 + (np.arange(h) // 100 % 3)[:, None]
    hi_z[..., 0] = 1.0 + (np.arange(H) * h // H // 100 % 3)[:, None]
    handle = bendy.Upscale()
    out = handle.apply(upload(bendy, color), 1, H, lo=(None, None, upload(bendy, lo_z)), hi=(None, None, upload(bendy, hi_z)))
    st = handle.poll()
    want, det = u.upscale(color, 1, 1, H, lo=(None, None, lo_z), hi=(None, None, hi_z), details=True)
    assert np.array_equal(out.numpy(), want) and (st.tier2, st.tier3, st.pixels) == det["counts"]


def test_handle_serves_frames_of_changing_size(bendy):
    handle = bendy.Upscale()
    P = dict(sigma_depth=0.3, normal_squarings=1)

    def call(hd, w, h, W, H):
        color, lo, hi = frames(w, h, W, H, (1, 4, 1), True)
        return check_call(bendy, hd, color, 3, lo, hi, W, H, **P)

    first = call(handle, 16, 17, 45, 35)
    call(handle, 8, 8, 32, 32)
    call(handle, 1, 1, 5, 3)
    assert handle.poll().pixels == 15
    assert np.array_equal(call(handle, 16, 17, 45, 35), first)
    assert np.array_equal(call(bendy.Upscale(), 16, 17, 45, 35), first)                     # a fresh handle agrees
    # out= is written in place, the inputs are left alone, the handle's own parameters hold
    handle = bendy.Upscale(**P)
    color, lo, hi = frames(16, 17, 45, 35, (1, 4, 1), True)
    buf, gl, gh = upload(bendy, color, 3), upload_guides(bendy, lo), upload_guides(bendy, hi)
    out = bendy.Buffer.new(45, 35)
    assert handle.apply(buf, 45, 35, lo=gl, hi=gh, out=out) is out and np.array_equal(out.numpy(), first)
    assert np.array_equal(buf.numpy(), color, equal_nan=True) and all(np.array_equal(b.numpy(), g[0], equal_nan=True) for b, g in zip(gl + gh, lo + hi))
    assert out.samples == 1 and out.color_space == buf.color_space
    for bad in (dict(lo=gl, hi=(gh[0], None, gh[2])), dict(lo=gh, hi=gh), dict(lo=gl, hi=gh, out=bendy.Buffer.new(44, 35))):
        with pytest.raises(bendy.BendyError):
            handle.apply(buf, 45, 35, **bad)
    with pytest.raises(bendy.BendyError) as e:
        handle.apply(buf, 15, 35)
    assert "bt_resample" in str(e.value)


@pytest.fixture(scope="module")
def rendered(bendy):
    """scene and cornell2 at 45x35 x 4 samples with their guides, and the guides of 1 sample at 90x70:
    (colour and guide Buffers, hi guide Buffers, the colour's host copy, the scene handle, the camera)."""
    import torch
    out = {}
    for name in ("scene", "cornell2"):
        sc, cam = gpu_scene(bendy, name, 45, 35)
        bufs = [bendy.Buffer.new(45, 35) for _ in range(4)]
        bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4)).render_guided(sc, cam, bendy.RenderConfig.with_samples(4), *bufs, seed=0x5EED)
        hi = []
        for output in (bendy.Output.Albedo, bendy.Output.Normal, bendy.Output.Depth):
            b = bendy.Buffer.new(90, 70)
            bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4, output=output)).render(sc, cam, bendy.RenderConfig.with_samples(1), b, seed=0xABC)
            hi.append(b)
        torch.cuda.synchronize()
        out[name] = (bufs, tuple(hi), bufs[0].numpy().copy(), sc, cam)
    return out


def host_guides(bufs):
    return tuple((b.numpy().copy(), b.samples) for b in bufs)


@pytest.mark.parametrize("name", ["scene", "cornell2"])
def test_renders_and_other_stages_are_left_alone(bendy, rendered, name):
    """A render on the same scene handle, its preview, display, glare and resample outputs are bit-identical before and after
    apply calls."""
    import torch
    bufs, hi, host, sc, cam = rendered[name]
    tr, rc = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4)), bendy.RenderConfig.with_samples(4)

    def everything():
        again = bendy.Buffer.new(45, 35)
        tr.render(sc, cam, rc, again, seed=0x5EED)
        torch.cuda.synchronize()
        return [again.numpy().copy(), again.preview(), bendy.Display().present(again), bendy.Glare().apply(again).numpy().copy(),
                bendy.Resample().apply(again, 90, 70).numpy().copy(), bendy.Resample(filter="tent").apply(again, 90, 70).numpy().copy()]

    before = everything()
    assert np.array_equal(before[0], host)
    handle = bendy.Upscale()
    lo_h, hi_h = host_guides(bufs[1:]), host_guides(hi)
    for p in (dict(), dict(sigma_depth=0.3, sigma_albedo=0.03, normal_squarings=0, min_weight=0.1), dict(normal_squarings=6, max_value=0.5)):
        out = handle.apply(bufs[0], 90, 70, lo=tuple(bufs[1:]), hi=hi, **p)
        st = handle.poll()
        want, det = u.upscale(host, 4, 90, 70, lo=lo_h, hi=hi_h, details=True, **{**u.DEFAULTS, **p})
        assert np.array_equal(out.numpy(), want) and (st.tier2, st.tier3, st.pixels) == det["counts"], p
    after = everything()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(bufs[0].numpy(), host)                  # apply does not write its input


@pytest.mark.parametrize("name", ["scene", "cornell2"])
def test_upscale_then_glare(bendy, rendered, name):
    """Glare().apply(Upscale().apply(...)) is the glare's restatement applied to the upscale's: the stage hands on a mean."""
    bufs, hi, host, _, _ = rendered[name]
    lo_h, hi_h = host_guides(bufs[1:]), host_guides(hi)
    for p, q in ((dict(), dict()), (dict(sigma_depth=0.3, normal_squarings=1), dict(strength=0.5, levels=3, spread=2.0))):
        got = bendy.Glare().apply(bendy.Upscale().apply(bufs[0], 90, 70, lo=tuple(bufs[1:]), hi=hi, **p), **q)
        want = glare_ref.glare(u.upscale(host, 4, 90, 70, lo=lo_h, hi=hi_h, **{**u.DEFAULTS, **p}), 1, **{**glare_ref.DEFAULTS, **q})
        assert got.samples == 1 and np.array_equal(got.numpy(), want), (p, q)


# ---- it helps, or it does not -------------------------------------------------------------------------------------------------

def rel_mse(x, y):
    """mean((x - y)^2 / (y^2 + 0.01)), DESIGN.md 11."""
    x, y = x[..., :3].astype(np.float64), y[..., :3].astype(np.float64)
    return float(np.mean((x - y) ** 2 / (y ** 2 + 0.01)))


def quality(bendy, name, w, h, W, H, params=None):
    """relMSE against a truth of 256 x Subpixel(2) samples at the shown size (seed 777) of a 4 x Subpixel(2) render at the small
    size (seed 0x5EED) shown through the resample stage's tent and through this stage, the hi guides 1 x Subpixel(2) (seed 0xABC)."""
    import torch
    cfg = dict(chunks_x=8, chunks_y=4)
    sc, cam = gpu_scene(bendy, name, W, H)                     # the aspect of the shown frame, for every render
    lo = [bendy.Buffer.new(w, h) for _ in range(4)]
    bendy.Tracer.with_config(bendy.Config(**cfg)).render_guided(sc, cam, bendy.RenderConfig(samples=4, subsample=bendy.Subsample(2)), *lo, seed=0x5EED)
    hi = []
    for output in (bendy.Output.Albedo, bendy.Output.Normal, bendy.Output.Depth):
        b = bendy.Buffer.new(W, H)
        bendy.Tracer.with_config(bendy.Config(output=output, **cfg)).render(sc, cam, bendy.RenderConfig(samples=1, subsample=bendy.Subsample(2)), b, seed=0xABC)
        hi.append(b)
    truth = bendy.Buffer.new(W, H)
    bendy.Tracer.with_config(bendy.Config(**cfg)).render(sc, cam, bendy.RenderConfig(samples=256, subsample=bendy.Subsample(2)), truth, seed=777)
    torch.cuda.synchronize()
    y = truth.mean()
    handle = bendy.Upscale(**(params or {}))
    guided = handle.apply(lo[0], W, H, lo=tuple(lo[1:]), hi=tuple(hi))
    st = handle.poll()
    tent = bendy.Resample(filter="tent").apply(lo[0], W, H)
    return dict(guided=rel_mse(guided.numpy(), y), tent=rel_mse(tent.numpy(), y), tier2=st.tier2 / st.pixels, tier3=st.tier3 / st.pixels)


# relMSE(guided) / relMSE(tent) as the stage's definition was prototyped in float32 numpy over CPU-oracle renders with the same
# seeds, sample counts and sizes (DESIGN.md 19 has the table): 0.019, 0.004 and 0.97.  GPU renders equal the oracle's bit for bit,
# so the figures should come again; the bound adds the 25 % DESIGN.md 11 and 14 give their ratios for seed-to-seed spread.  Only a
# row whose ratio x 1.25 is below 1 has a bound of its own; `scene`, where the error is fireflies and lost sharpness that no
# upsampler returns, is printed and held to "no worse than the tent by more than that spread".
# measured on an MI355X: 0.0189 (4.191 -> 0.0793), 0.0044 (8.442 -> 0.03755), 0.9685 (0.02506 -> 0.02427) -- the prototype's figures.
HELPS = [("cornell2", 64, 64, 128, 128, 0.019 * 1.25), ("cornell", 32, 32, 128, 128, 0.0045 * 1.25), ("scene", 64, 36, 128, 72, 0.97 * 1.25)]


@pytest.mark.parametrize("name,w,h,W,H,bound", HELPS)
def test_it_helps_a_small_render_shown_large(bendy, name, w, h, W, H, bound):
    r = quality(bendy, name, w, h, W, H)
    print(f"{name} {w}x{h} -> {W}x{H}: relMSE tent {r['tent']:.4g}, guided {r['guided']:.4g}, ratio {r['guided'] / r['tent']:.4f}; "
          f"tier 2 {100 * r['tier2']:.2f} %, tier 3 {100 * r['tier3']:.2f} %")
    assert r["guided"] / r["tent"] <= bound
