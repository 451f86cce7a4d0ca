"""The compare stage (EXTENSION) on the GPU against tests/compare_ref.py: the stats with `==`, the three planes, the
tail and the map with array_equal; a frame of more tile rows than a grid axis takes; a handle that serves frames of changing size;
same-pointer frames; renders and the other stages left alone; and that it measures what it says on a converging render.  Frames are
uploaded, not rendered, except where a test says so."""
import math

import numpy as np
import pytest

import compare_ref as c
from helpers import gpu_scene
from test_compare_host import SHAPES, TAILS, cases, check_stats

pytestmark = pytest.mark.gpu
f32 = np.float32


def upload(bendy, frame, samples=1):
    import torch
    frame = np.ascontiguousarray(frame, dtype=f32)
    buf = bendy.Buffer.new(frame.shape[1], frame.shape[0])
    buf.data.copy_(torch.from_numpy(frame))
    buf.samples = samples
    return buf


def check_call(bendy, handle, X, Y, nx, ny, scale=1.0, **p):
    """One measure against the restatement: the stats, the three planes, the tail at three fractions and the map."""
    st = handle.measure(upload(bendy, X, nx), upload(bendy, Y, ny), **p)
    want = c.measure(X, Y, nx, ny, **{**c.DEFAULTS, **p})
    check_stats(st, want)
    E = handle.plane("E")
    assert np.array_equal(E, want["E"]) and np.array_equal(np.signbit(E), np.signbit(want["E"]))      # no pixel is exempt
    assert np.array_equal(handle.plane("v"), want["v"]) and np.array_equal(handle.plane("s"), want["s"])
    for f in TAILS:
        assert handle.tail(f) == c.tail(want["E"], f), f
    assert np.array_equal(handle.map(scale).cpu().numpy(), c.error_map(want["E"], scale))
    check_stats(handle.poll(), want)                                   # the tail and the map left the results alone
    return st


@pytest.mark.parametrize("w,h", SHAPES)
def test_device_is_the_restatement(bendy, w, h):
    handle = bendy.Compare()
    for n, (X, Y, nx, ny, p) in enumerate(cases(w, h)):
        check_call(bendy, handle, X, Y, nx, ny, scale=(1.0, 0.01, 1e30)[n % 3], **p)


def test_more_tile_rows_than_a_grid_axis_takes(bendy):
    """The grid of tiles is one-dimensional: a frame of 65 538 tile rows, beyond what grid.y takes, is no special case."""
    h = 65537 * 16 + 3
    assert h == 1048595
    rng = np.random.default_rng(6)
    Y = np.ones((h, 1, 4), dtype=f32)
    Y[..., :3] = np.exp2(rng.uniform(-4.0, 4.0, size=(h, 1, 3))).astype(f32)
    X = Y.copy()
    X[..., :3] = (Y[..., :3] * (1.0 + 0.1 * rng.standard_normal((h, 1, 3)))).astype(f32)
    X[h - 2, 0, 1] = np.nan
    handle = bendy.Compare()
    st = handle.measure(upload(bendy, X), upload(bendy, Y))
    want = c.measure(X, Y)
    check_stats(st, want)
    assert st.nonfinite == 1 and np.array_equal(handle.plane("s"), want["s"])
    assert handle.tail(0.01) == c.tail(want["E"], 0.01)


def test_handle_serves_frames_of_changing_size(bendy):
    handle = bendy.Compare(epsilon=1e-4)

    def call(hd, w, h):
        X, Y = c.make_pair(w, h, seed=w + h, noise=0.3, nx=3, ny=4, poison="nonfinite")
        st = check_call(bendy, hd, X, Y, 3, 4, epsilon=1e-4)
        return [getattr(st, k) for k in c.FIELDS], hd.plane("E"), hd.plane("v"), hd.plane("s"), hd.tail(0.1), hd.map(0.5).cpu().numpy()

    first = call(handle, 16, 17)
    call(handle, 64, 36)
    call(handle, 1, 1)
    assert handle.poll().pixels == 1
    for other in (call(handle, 16, 17), call(bendy.Compare(), 16, 17)):                # the first again; a fresh handle
        assert other[0] == first[0] and other[4] == first[4] and all(np.array_equal(a, b) for a, b in zip(other[1:4] + other[5:], first[1:4] + first[5:]))


def test_same_pointer_frames_give_the_identity(bendy):
    X, _ = c.make_pair(45, 35, seed=8, nx=3, poison="nonfinite")
    buf = upload(bendy, X, 3)
    handle = bendy.Compare()
    st = handle.measure(buf, buf)
    assert (st.mse, st.rel_mse, st.max_abs, st.max_index, st.ssim, st.psnr) == (0.0, 0.0, 0.0, 0, 1.0, math.inf)
    assert st.nonfinite == 2 and st.valid == 45 * 35 - 2 and (handle.plane("s") == 1.0).all()
    assert handle.tail(0.01) == (0.0, 0.0) and handle.tail(1.0) == (0.0, 0.0)
    assert np.array_equal(buf.numpy(), X, equal_nan=True)               # measure does not write its inputs


@pytest.mark.parametrize("name", ["scene", "cornell2"])
def test_renders_and_other_stages_are_left_alone(bendy, name):
    """A render on the same scene handle, its preview, display, glare, resample, despeckle and upscale outputs are bit-identical
    before and after measure calls."""
    import torch
    sc, cam = gpu_scene(bendy, name, 45, 35)
    tr, rc = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4)), bendy.RenderConfig.with_samples(4)

    def everything():
        again = bendy.Buffer.new(45, 35)
        tr.render(sc, cam, rc, again, seed=0x5EED)
        torch.cuda.synchronize()
        return again, [again.numpy().copy(), again.preview(), bendy.Display().present(again), bendy.Glare().apply(again).numpy().copy(),
                       bendy.Resample().apply(again, 90, 70).numpy().copy(), bendy.Despeckle().apply(again).numpy().copy(),
                       bendy.Upscale().apply(again, 90, 70).numpy().copy()]

    buf, before = everything()
    handle = bendy.Compare()
    other = bendy.Glare().apply(buf)
    for p in (dict(), dict(epsilon=1e-4, peak=4.0)):
        st = handle.measure(other, buf, **p)
        check_stats(st, c.measure(other.numpy(), before[0], 1, 4, **{**c.DEFAULTS, **p}))
        handle.tail(0.01)
        handle.map(0.1)
    _, after = everything()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(buf.numpy(), before[0])


# relMSE and SSIM of cornell2 at 64 x 64, 1 / 4 / 16 / 64 samples x Subpixel(2) (seed 0x5EED) against 256 x Subpixel(2) (seed
# 0xBEEF), as the restatement gives them on CPU-oracle renders, which GPU renders equal bit for bit (DESIGN.md 20 has the table)
def test_it_measures(bendy):
    import torch
    sc, cam = gpu_scene(bendy, "cornell2", 64, 64)
    tr = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4))
    truth = bendy.Buffer.new(64, 64)
    tr.render(sc, cam, bendy.RenderConfig(samples=256, subsample=bendy.Subsample(2)), truth, seed=0xBEEF)
    handle, rows = bendy.Compare(), []
    for spp in (1, 4, 16, 64):
        buf = bendy.Buffer.new(64, 64)
        tr.render(sc, cam, bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(2)), buf, seed=0x5EED)
        torch.cuda.synchronize()
        st = handle.measure(buf, truth)
        formula = c.rel_mse_numpy(buf.mean(), truth.mean())
        print(f"cornell2 64x64 {spp:3d} x Subpixel(2): relMSE {st.rel_mse:.6g} (numpy formula {formula:.6g}), SSIM {st.ssim:.6f}, "
              f"PSNR {st.psnr:.3f}, tail(1 %) {handle.tail(0.01)[0]:.4f}")
        assert st.nonfinite == 0 and math.isclose(st.rel_mse, formula, rel_tol=1e-10)
        rows.append(st)
    assert all(a.rel_mse > b.rel_mse for a, b in zip(rows, rows[1:]))       # strictly decreasing
    assert all(a.ssim < b.ssim for a, b in zip(rows, rows[1:]))             # strictly increasing
