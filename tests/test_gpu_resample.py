"""The resample stage (EXTENSION) on the GPU against tests/resample_ref.py, bit for bit: the output and the
intermediate plane P (so the pass that is wrong is named), with the library's own tables; a handle that shrinks and grows;
renders left alone; and glare, resample and the display stage in a row.  Frames are uploaded, not rendered, except where a test
says so.  Both forms of the kernels (staged in LDS, direct; bt_resample.hpp's BT_RESAMPLE_LDS) pass this file unchanged."""
import numpy as np
import pytest

import display_ref
import glare_ref as g
import resample_ref as r
from helpers import gpu_scene
from test_gpu_glare import upload
from test_resample_host import SAMPLES, library_tables
from test_resample_ref import FILTERS, SHAPES

pytestmark = pytest.mark.gpu
f32 = np.float32


def check_call(bendy, handle, frame, samples, W, H, **p):
    """One apply against the restatement fed the handle's own tables: P first, then the output."""
    out = handle.apply(upload(bendy, frame, samples), W, H, **p)
    assert out.samples == 1 and (out.width, out.height) == (W, H)
    got = out.numpy()
    q = {**r.DEFAULTS, **{k: getattr(handle.params, k) for k in r.DEFAULTS}, **p}
    want, P = r.resample(frame, samples, W, H, plane=True, tables=library_tables(handle), **q)
    plane = handle.plane()
    assert plane.shape == P.shape and np.array_equal(plane, P), ("P", q, samples, np.argwhere(plane != P)[:4])
    assert np.array_equal(got, want), (q, samples, np.argwhere(got != want)[:4])          # no pixel is exempt
    return got


@pytest.mark.parametrize("src,dst", SHAPES)
def test_device_is_the_restatement(bendy, src, dst):
    (w, h), (W, H) = src, dst
    frame = r.make_frame(w, h, seed=w * 1000 + h)
    for filt in FILTERS:
        handle = bendy.Resample(filter=filt)
        for n in SAMPLES:
            got = check_call(bendy, handle, frame, n, W, H)
            assert np.isfinite(got).all()
            assert np.array_equal(got, handle.host(frame, n, W, H))                       # and the host entry point's
        check_call(bendy, handle, frame, 3, W, H, clamp_negative=0)
        check_call(bendy, handle, frame, 1, W, H, max_value=0.5)
        handle.close()


@pytest.mark.parametrize("src,dst,filt", [((600, 9), (70, 9), r.TENT), ((9, 500), (9, 70), r.LANCZOS3), ((2100, 3), (100, 2), r.LANCZOS3),
                                          ((127, 130), (1, 2), r.BOX), ((40, 30), (1000, 9), r.MITCHELL), ((496, 4), (96, 4), r.LANCZOS3),
                                          ((498, 4), (96, 4), r.LANCZOS3)])
def test_every_path_of_the_horizontal_pass(bendy, src, dst, filt):
    """The horizontal pass stages its source span in LDS where a row has six taps and more and the 32 outputs of a workgroup take at
    most 192 source texels, and loads every tap from memory elsewhere: ratios on both sides of each limit (496 -> 96 takes 192
    texels, 498 -> 96 takes 193), few taps, and the largest tap counts there are.  The same answer either way."""
    (w, h), (W, H) = src, dst
    handle = bendy.Resample(filter=filt)
    check_call(bendy, handle, r.make_frame(w, h, seed=w + h), 3, W, H)


def test_handle_shrinks_grows_and_leaves_no_residue(bendy):
    handle = bendy.Resample(filter="lanczos3")
    a, b, c = r.make_frame(45, 35, seed=1), r.make_frame(16, 17, seed=2), r.make_frame(1, 1, seed=3)
    first = check_call(bendy, handle, a, 3, 16, 17)
    check_call(bendy, handle, b, 1, 45, 35)
    check_call(bendy, handle, c, 1, 5, 3)
    assert np.array_equal(check_call(bendy, handle, a, 3, 16, 17), first)
    assert np.array_equal(check_call(bendy, bendy.Resample(filter="lanczos3"), a, 3, 16, 17), first)           # a fresh handle agrees
    check_call(bendy, handle, a, 3, 16, 17, filter="box")                                                       # the table is replaced
    assert np.array_equal(check_call(bendy, handle, a, 3, 16, 17), first)
    # out= is written in place; the input is left alone
    buf = upload(bendy, a, 3)
    out = bendy.Buffer.new(16, 17)
    assert handle.apply(buf, 16, 17, out=out) is out and np.array_equal(out.numpy(), first) and np.array_equal(buf.numpy(), a, equal_nan=True)
    with pytest.raises(bendy.BendyError):
        handle.apply(buf, 16, 17, out=bendy.Buffer.new(17, 16))
    with pytest.raises(bendy.BendyError):
        handle.apply(buf, 45, 35, out=buf)
    with pytest.raises(bendy.BendyError):
        handle.apply(buf, 0, 35)


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
    """A render on the same scene handle, its preview, its display and its glare are bit-identical before and after apply calls."""
    import torch
    buf, host, sc, cam = rendered[name]
    tr, rc = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4)), bendy.RenderConfig.with_samples(4)

    def everything():
        again = bendy.Buffer.new(45, 35)
        tr.render(sc, cam, rc, again, seed=0x5EED)
        torch.cuda.synchronize()
        return [again.numpy().copy(), again.preview(), bendy.Display().present(again), bendy.Glare().apply(again).numpy()]

    before = everything()
    assert np.array_equal(before[0], host)
    handle = bendy.Resample()
    for W, H, p in ((90, 70, dict()), (16, 17, dict(filter="lanczos3")), (45, 35, dict(filter="tent"))):
        check_call(bendy, handle, host, 4, W, H, **p)
        handle.apply(buf, W, H, **p)
    after = everything()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(buf.numpy(), host)                     # apply does not write its input


@pytest.mark.parametrize("name", ["scene", "cornell2"])
def test_glare_then_resample_then_present(bendy, oracle, rendered, name):
    """Display().present(Resample().apply(Glare().apply(buf), 90, 70)) is the display stage's restatement applied to the chain of
    the other two restatements, with the GPU's own exposure multiplier."""
    buf, host, _, _ = rendered[name]
    d = bendy.Display()
    shown = d.present(bendy.Resample().apply(bendy.Glare().apply(buf), 90, 70))
    _, mult = d.exposure()
    resampled = r.resample(g.glare(host, buf.samples, **g.DEFAULTS), 1, 90, 70, **r.DEFAULTS)
    want = oracle.preview(display_ref.shown_frame(resampled, 1, mult, display_ref.ACES), 1, int(buf.color_space))
    assert shown.shape == (70, 90, 4) and np.array_equal(shown, want), np.argwhere(shown != want)[:4]
    # the result is a mean in the input's colour space: preview() takes it as it is
    small = bendy.Resample(filter="box").apply(buf, 15, 7)
    assert small.color_space == buf.color_space and small.preview().shape == (7, 15, 4)
    assert np.array_equal(small.preview(), oracle.preview(r.resample(host, buf.samples, 15, 7, filter=r.BOX), 1, int(buf.color_space)))
