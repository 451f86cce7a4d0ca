"""bt_adaptive / bt_render_adaptive_device / Tracer.render_adaptive (EXTENSION): what is decided before the
device is touched.  Runs without a GPU; the pointers handed to the library here are dummies that a refused call never
dereferences.  (The one refusal that needs an earlier successful pass -- a changed pass size -- is in test_gpu_adaptive.py.)"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROOT, scene_path

INVALID_ARG, DEVICE, UNSUPPORTED, DONE, IN_PROGRESS = -1, -8, -9, 0, 1
FRAME = 0x1000                  # a non-NULL "device" address
W, H = 40, 24                   # 3 x 2 tiles
NEW = ["bt_adaptive_params_default", "bt_adaptive_new", "bt_adaptive_free", "bt_adaptive_reset", "bt_render_adaptive_device",
       "bt_adaptive_poll", "bt_adaptive_counts", "bt_adaptive_errors", "bt_debug_adaptive_moments",
       "bt_adaptive_resolve_device"]


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _setup(bendy, samples=2, output=0, render_output=None, n=0):
    from bendy_tracer_amd import api
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    rcfg = bendy.RenderConfig(samples=samples, subsample=bendy.Subsample(n),
                              output=None if render_output is None else bendy.Output(render_output))
    c, r = api._c_configs(bendy.Config(output=bendy.Output(output)), rcfg, 0)
    return api, sc, cam, c, r


def _params(api, **kw):
    p = api._CAdaptiveParams()
    api.lib.bt_adaptive_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _call(api, sc, cam, c, r, ad, p, frame=FRAME, scene=True, w=W, h=H):
    return api.lib.bt_render_adaptive_device(sc._h if scene else None, cam, C.byref(c) if c is not None else None,
                                             C.byref(r) if r is not None else None, ad._h if ad is not None else None,
                                             C.byref(p) if p is not None else None, C.c_void_p(frame) if frame else None,
                                             w, h, 1, None)


def _err(api):
    return api.lib.bt_last_error()


def test_symbols_are_declared_and_exported(bendy):
    from bendy_tracer_amd import api
    hdr = open(os.path.join(ROOT, "include", "bendy_hip.h")).read()
    for name in NEW:
        assert name in api.EXPORTS and hasattr(api.lib, name), name
        assert name + "(" in hdr, name
    assert "variance-driven adaptive sampling" in hdr and "bt_adaptive_stats" in hdr
    for name in ("Adaptive", "AdaptiveParams", "AdaptiveStats"):
        assert hasattr(bendy, name)
    assert hasattr(bendy.Tracer, "render_adaptive")


def test_defaults(bendy):
    from bendy_tracer_amd import api
    p = _params(api)
    assert p.eps == np.float32(1e-3)
    assert math.isfinite(p.threshold) and p.threshold > 0.0
    assert 1 <= p.min_samples <= p.max_samples
    api.lib.bt_adaptive_params_default(None)             # tolerated, like the other *_default functions
    q = bendy.AdaptiveParams()
    assert (np.float32(q.threshold), q.min_samples, q.max_samples, np.float32(q.eps)) == (p.threshold, p.min_samples, p.max_samples, p.eps)
    assert bendy.AdaptiveParams(threshold=0.5, max_samples=7).max_samples == 7


def test_handle_sizes_and_fresh_state_need_no_device(bendy):
    from bendy_tracer_amd import api
    ad = bendy.Adaptive(W, H)
    assert api.lib.bt_adaptive_counts(ad._h, None, 0) == 6                   # n == 0 asks for the size
    assert api.lib.bt_adaptive_errors(ad._h, None, 0) == 6
    assert api.lib.bt_debug_adaptive_moments(ad._h, None, 0) == W * H
    assert ad.counts().shape == (2, 3) and ad.counts().dtype == np.uint32 and not ad.counts().any()
    assert ad.errors().shape == (2, 3) and ad.errors().dtype == np.float32 and not ad.errors().any()
    assert ad.moments().shape == (H, W) and not ad.moments().any()
    part = np.full(4, 9, dtype=np.uint32)                                    # fewer than there are: that many are written
    assert api.lib.bt_adaptive_counts(ad._h, part.ctypes.data_as(C.POINTER(C.c_uint32)), 4) == 4 and not part.any()
    st = ad.poll()
    assert (st.active_tiles, st.tiles, st.min_count, st.max_count, st.pixel_samples, st.passes) == (6, 6, 0, 0, 0, 0)
    assert api.lib.bt_adaptive_poll(ad._h, None) == IN_PROGRESS
    ad.reset()
    assert ad.poll().active_tiles == 6
    for fn in (api.lib.bt_adaptive_counts, api.lib.bt_adaptive_errors, api.lib.bt_debug_adaptive_moments):
        assert fn(None, None, 0) == INVALID_ARG
        assert fn(ad._h, None, 3) == INVALID_ARG
    assert api.lib.bt_adaptive_reset(None) == INVALID_ARG and api.lib.bt_adaptive_poll(None, None) == INVALID_ARG
    assert not api.lib.bt_adaptive_new(0, 8) and not api.lib.bt_adaptive_new(8, 0)
    with pytest.raises(bendy.BendyError):
        bendy.Adaptive(0, 0)
    api.lib.bt_adaptive_free(None)


def test_null_arguments_are_refused_first(bendy):
    api, sc, cam, c, r = _setup(bendy)
    ad, p = bendy.Adaptive(W, H), _params(api)
    assert _call(api, sc, cam, c, r, ad, p, scene=False) == INVALID_ARG
    assert _call(api, sc, cam, None, r, ad, p) == INVALID_ARG
    assert _call(api, sc, cam, c, None, ad, p) == INVALID_ARG
    assert _call(api, sc, cam, c, r, None, p) == INVALID_ARG
    assert _call(api, sc, cam, c, r, ad, None) == INVALID_ARG
    assert _call(api, sc, cam, c, r, ad, p, frame=0) == INVALID_ARG
    # ... ahead of everything else
    sc.set_lens((0.0, 0.0, 0.0), 0.1, 0.1, 2.0)
    r.samples = 0
    c.output = 1
    assert _call(api, sc, cam, c, r, ad, _params(api, threshold=-1.0), frame=0, w=W + 1) == INVALID_ARG
    assert b"null" in _err(api)


@pytest.mark.parametrize("output", [1, 2, 3])
def test_effective_output_must_be_full(bendy, output):
    api, sc, cam, c, r = _setup(bendy, output=output)                        # Config.output
    ad = bendy.Adaptive(W, H)
    assert _call(api, sc, cam, c, r, ad, _params(api)) == INVALID_ARG and b"output" in _err(api)
    api, sc, cam, c, r = _setup(bendy, output=0, render_output=output)       # RenderConfig.output overrides it (mod.rs:220)
    assert _call(api, sc, cam, c, r, ad, _params(api)) == INVALID_ARG and b"output" in _err(api)
    # ahead of the frame size, the parameters, the lens and samples == 0
    api, sc, cam, c, r = _setup(bendy, samples=0, output=output)
    sc.set_lens((0.0, 0.0, 0.0), 0.1, 0.1, 2.0)
    assert _call(api, sc, cam, c, r, ad, _params(api, threshold=-1.0, min_samples=9, max_samples=1), w=W + 1) == INVALID_ARG
    assert b"output" in _err(api)
    api, sc, cam, c, r = _setup(bendy, samples=0, output=output, render_output=0)    # ... and a valid one passes this check
    assert _call(api, sc, cam, c, r, ad, _params(api)) == DONE


def test_refusals_come_in_the_documented_order(bendy):
    api, sc, cam, c, r = _setup(bendy, samples=0)
    sc.set_lens((0.0, 0.0, 0.0), 0.1, 0.1, 2.0)
    ad = bendy.Adaptive(W, H)
    bad = dict(threshold=-1.0, min_samples=9, max_samples=1)
    # the frame size, ahead of the parameters
    for w, h in ((W + 1, H), (W, H - 1), (H, W)):
        assert _call(api, sc, cam, c, r, ad, _params(api, **bad), w=w, h=h) == INVALID_ARG
        assert b"adaptive handle of" in _err(api)
    # the threshold, ahead of min > max
    for t in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert _call(api, sc, cam, c, r, ad, _params(api, threshold=t, min_samples=9, max_samples=1)) == INVALID_ARG
        assert b"threshold" in _err(api)
    # min > max, ahead of the lens
    assert _call(api, sc, cam, c, r, ad, _params(api, min_samples=9, max_samples=1)) == INVALID_ARG
    assert b"min_samples" in _err(api)
    # the lens, ahead of samples == 0
    assert _call(api, sc, cam, c, r, ad, _params(api)) == UNSUPPORTED and b"lens" in _err(api)
    sc.clear_lens()
    assert _call(api, sc, cam, c, r, ad, _params(api)) == DONE               # mod.rs:186-188; the device is not needed for it
    assert _call(api, sc, cam, c, r, ad, _params(api, threshold=0.0, min_samples=5, max_samples=5)) == DONE   # both limits are valid
    assert ad.poll().passes == 0                                             # nothing of this counted as a pass


def test_resolve_refusals(bendy):
    from bendy_tracer_amd import api
    ad = bendy.Adaptive(W, H)
    f = api.lib.bt_adaptive_resolve_device
    assert f(None, C.c_void_p(FRAME), C.c_void_p(2 * FRAME), None) == INVALID_ARG
    assert f(ad._h, None, C.c_void_p(2 * FRAME), None) == INVALID_ARG
    assert f(ad._h, C.c_void_p(FRAME), None, None) == INVALID_ARG
    assert f(ad._h, C.c_void_p(FRAME), C.c_void_p(FRAME), None) == INVALID_ARG and b"out must not be rgba" in _err(api)


def test_valid_call_without_a_device_is_a_device_error(bendy):
    if _have_gpu():
        pytest.skip("a GPU is present")            # (the dummy frame would be written to)
    api, sc, cam, c, r = _setup(bendy)
    ad = bendy.Adaptive(W, H)
    assert _call(api, sc, cam, c, r, ad, _params(api)) == DEVICE
    assert ad.poll().passes == 0 and not ad.counts().any()


def test_python_method_refuses_host_buffers(bendy):
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    ad = bendy.Adaptive(16, 8)
    cpu = bendy.Buffer.new(16, 8, device="cpu")
    with pytest.raises(bendy.BendyError) as e:
        bendy.Tracer.new().render_adaptive(sc, cam, bendy.RenderConfig.with_samples(1), cpu, ad)
    assert e.value.code == INVALID_ARG and cpu.samples == 0
    with pytest.raises(bendy.BendyError):
        ad.resolve(cpu)
    with pytest.raises(TypeError):
        bendy.Adaptive(16, 8, sigma=1.0)                                     # keywords are AdaptiveParams fields
