"""The glare stage (EXTENSION) on the GPU against tests/glare_ref.py, bit for bit: the output, every plane A_k of
the pyramid (so a wrong level is named), a handle that shrinks and grows, renders left alone, and glare ahead of the display
stage.  Frames are uploaded, not rendered, except where a test says so."""
import os

import numpy as np
import pytest

import display_ref
import glare_ref as g
from conftest import GOLDEN
from helpers import gpu_scene
from test_glare_host import GOLDEN_FRAMES, SHAPES, settings

pytestmark = pytest.mark.gpu
f32 = np.float32


def upload(bendy, frame, samples=1):
    import torch
    frame = np.ascontiguousarray(frame, dtype=f32)
    buf = bendy.Buffer.new(frame.shape[1], frame.shape[0])
    buf.data.copy_(torch.from_numpy(frame))
    buf.samples = samples
    return buf


def check_call(bendy, handle, frame, samples, planes=True, **p):
    """One apply against the restatement: the output, and (planes) every A_k, coarsest first so the first wrong level is the cause."""
    out = handle.apply(upload(bendy, frame, samples), **p)
    assert out.samples == 1
    got = out.numpy()
    want, A = g.glare(frame, samples, planes=True, **{**g.DEFAULTS, **p})
    if planes:
        for k in range(len(A), 0, -1):
            pk = handle.plane(k)
            assert pk.shape == A[k - 1].shape and np.array_equal(pk, A[k - 1]), ("A_%d" % k, p, samples, np.argwhere(pk != A[k - 1])[:4])
        with pytest.raises(bendy.BendyError):
            handle.plane(len(A) + 1)
    assert np.array_equal(got, want), (p, samples, np.argwhere(got != want)[:4])          # no pixel is exempt
    return got


@pytest.mark.parametrize("w,h", SHAPES)
def test_device_is_the_restatement(bendy, w, h):
    handle = bendy.Glare()
    frame = g.make_frame(w, h, seed=w * 1000 + h)
    for levels, samples, spread, strength in settings():
        got = check_call(bendy, handle, frame, samples, levels=levels, spread=spread, strength=strength)
        assert np.isfinite(got[..., :3]).all()


@pytest.mark.parametrize("name", GOLDEN_FRAMES)
def test_device_on_golden_frames(bendy, name):
    handle = bendy.Glare()
    frame = np.load(os.path.join(GOLDEN, name + ".npz"))["iterative"]
    for levels, samples, spread, strength in settings():
        check_call(bendy, handle, frame, samples, levels=levels, spread=spread, strength=strength)
    check_call(bendy, handle, frame, 4)                          # the defaults
    check_call(bendy, handle, frame, 4, max_value=0.5)


def test_handle_shrinks_grows_and_leaves_no_residue(bendy):
    P = dict(levels=16, spread=2.0, strength=0.5)
    handle = bendy.Glare()
    mid, small, large = g.make_frame(45, 35, seed=1), g.make_frame(3, 5, seed=2), g.make_frame(300, 200, seed=3)
    first = check_call(bendy, handle, mid, 3, **P)
    check_call(bendy, handle, small, 1, **P)
    check_call(bendy, handle, large, 4, **P)
    check_call(bendy, handle, np.full((1, 1, 4), 2.5, dtype=f32), 1, **P)          # L = 0: no plane at all
    with pytest.raises(bendy.BendyError):
        handle.plane(1)
    assert np.array_equal(check_call(bendy, handle, mid, 3, **P), first)
    assert np.array_equal(check_call(bendy, bendy.Glare(), mid, 3, **P), first)             # a fresh handle agrees
    handle = bendy.Glare(**P)                                                               # the handle's own parameters
    # out= is written in place; the input is left alone
    buf = upload(bendy, mid, 3)
    out = bendy.Buffer.new(45, 35)
    assert handle.apply(buf, out=out) is out and np.array_equal(out.numpy(), first) and np.array_equal(buf.numpy(), mid, equal_nan=True)
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
    handle = bendy.Glare()
    for p in (dict(), dict(levels=2, strength=1.0), dict(levels=0)):
        check_call(bendy, handle, host, 4, **p)
        handle.apply(buf, **p)
    after = everything()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(buf.numpy(), host)                     # apply does not write its input


@pytest.mark.parametrize("name", ["scene", "cornell2"])
def test_glare_then_present(bendy, oracle, rendered, name):
    """Display().present(Glare().apply(buf)) is the display stage's restatement applied to the glare's restatement, with the
    GPU's own exposure multiplier."""
    buf, host, _, _ = rendered[name]
    d = bendy.Display()
    for p in (dict(), dict(strength=0.5, levels=3, spread=2.0)):
        shown = d.present(bendy.Glare().apply(buf, **p))
        _, mult = d.exposure()
        glared = g.glare(host, buf.samples, **{**g.DEFAULTS, **p})
        want = oracle.preview(display_ref.shown_frame(glared, 1, mult, display_ref.ACES), 1, int(buf.color_space))
        assert np.array_equal(shown, want), (p, np.argwhere(shown != want)[:4])
    assert not np.array_equal(shown, d.present(buf))              # and the glare is visible in the shown frame
