"""The upscale stage (EXTENSION) on a machine without a GPU: the defaults, the handle's life cycle, what
bt_upscale_device refuses before it touches the device and in which order, and BT_ERR_DEVICE for a valid call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FAKE = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000]   # never dereferenced: every call fails before the device
NAMES = ["bt_upscale_params_default", "bt_upscale_new", "bt_upscale_free", "bt_upscale_device", "bt_upscale_poll",
         "bt_debug_upscale_weights", "bt_debug_upscale_plane", "bt_debug_upscale_host"]
GOOD = dict(sigma_depth=0.1, sigma_albedo=0.1, normal_squarings=3, min_weight=0.01, max_value=65536.0)
NAN, INF = float("nan"), float("inf")
GUIDES = ("albedo", "normal", "depth")


def _guides(bendy, spec, base):
    """spec: {guide name: sample count, or (pointer, sample count)} -> bt_upscale_guides."""
    g = bendy.api._CUpscaleGuides()
    for k, name in enumerate(GUIDES):
        if name in spec:
            ptr, n = spec[name] if isinstance(spec[name], tuple) else (FAKE[base + k], spec[name])
            setattr(g, name, ptr)
            setattr(g, name + "_samples", n)
    return g


def _call(bendy, g, src=FAKE[0], samples=1, w=8, h=8, lo=None, hi=None, dst=FAKE[1], W=16, H=16, params=None, **fields):
    lib = bendy.api.lib
    p = None
    if params is not None or fields:
        p = C.byref(bendy.api._CUpscaleParams(*{**GOOD, **(params or {}), **fields}.values()))
    gl = C.byref(_guides(bendy, lo, 2)) if lo is not None else None
    gh = C.byref(_guides(bendy, hi, 5)) if hi is not None else None
    rc = lib.bt_upscale_device(g, src, samples, w, h, gl, gh, dst, W, H, p, None)
    return rc, lib.bt_last_error().decode()


def test_symbols_and_defaults(bendy):
    api = bendy.api
    hdr = open(os.path.join(ROOT, "include", "bendy_hip.h")).read()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(api.lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    for name in ("bt_upscale_params", "bt_upscale_guides", "bt_upscale_stats", "bt_upscale"):
        assert re.search(r"\}\s*%s;|typedef struct %s %s;" % (name, name, name), hdr), name
    p = api._CUpscaleParams()
    api.lib.bt_upscale_params_default(C.byref(p))
    api.lib.bt_upscale_params_default(None)
    got = {k: getattr(p, k) for k, _ in api._CUpscaleParams._fields_}
    assert got == {k: (v if isinstance(v, int) else float(np.float32(v))) for k, v in GOOD.items()}
    assert C.sizeof(api._CUpscaleParams) == 20 and C.sizeof(api.UpscaleStats) == 16 and C.sizeof(api._CUpscaleGuides) == 48
    q = bendy.UpscaleParams(normal_squarings=5, sigma_depth=0.25)
    assert (q.sigma_depth, q.sigma_albedo, q.normal_squarings, q.min_weight, q.max_value) == (
        0.25, float(np.float32(0.1)), 5, float(np.float32(0.01)), 65536.0)
    assert q._c().normal_squarings == 5 and q._c().sigma_depth == 0.25
    # the C++ delegate is declared next to the others
    hpp = open(os.path.join(ROOT, "include", "bendy_tracer.hpp")).read()
    assert "class Upscale" in hpp and "bt_upscale_device(h_" in hpp


def test_new_free_and_poll_without_a_device(bendy):
    lib = bendy.api.lib
    g = C.c_void_p(lib.bt_upscale_new())
    assert g
    st = bendy.UpscaleStats()
    assert lib.bt_upscale_poll(g, C.byref(st)) == -1 and "before" in lib.bt_last_error().decode()      # no call yet
    assert lib.bt_upscale_poll(g, None) == -1 and lib.bt_upscale_poll(None, C.byref(st)) == -1
    assert lib.bt_debug_upscale_weights(g, 0, None, None, None, None) == -1 and lib.bt_debug_upscale_weights(g, 2, None, None, None, None) == -1
    assert lib.bt_debug_upscale_plane(g, 0, None, 0) == -1 and lib.bt_debug_upscale_plane(g, 3, None, 0) == -1
    lib.bt_upscale_free(g)
    lib.bt_upscale_free(None)
    h = bendy.Upscale(sigma_albedo=0.5, normal_squarings=0)
    assert (h.params.sigma_albedo, h.params.normal_squarings, h.params.min_weight) == (0.5, 0, float(np.float32(0.01)))
    with pytest.raises(bendy.BendyError) as e:
        h.poll()
    assert e.value.code == -1
    with pytest.raises(bendy.BendyError) as e:
        h.apply(bendy.Buffer(4, 4, device="cpu"), 8, 8)
    assert e.value.code == -1 and "host-buffer" in str(e.value)
    h.close()
    h.close()


def test_validation_order(bendy):
    """Each rule alone, and each rule together with a violation of every later one: the earlier rule's message wins."""
    lib = bendy.api.lib
    g = C.c_void_p(lib.bt_upscale_new())
    both = dict(lo=dict(albedo=1, normal=1, depth=1), hi=dict(albedo=1, normal=1, depth=1))
    # (arguments that break the rule, a word of its message), in the header's order
    rules = [
        ([dict(g=None), dict(src=None), dict(dst=None)], "null"),
        ([dict(samples=0)], "0 samples"),
        ([dict(w=0), dict(h=0), dict(W=0), dict(H=0), dict(w=1 << 16, h=1 << 16, W=1 << 16, H=1 << 16), dict(W=1 << 31, H=1)], "zero-sized"),
        ([dict(W=7), dict(H=7), dict(w=17, h=17)], "bt_resample"),
        ([dict(dst=FAKE[0]), dict(dst=FAKE[3], **both), dict(dst=FAKE[7], **both)], "alias"),
        ([dict(lo=dict(albedo=1), hi=None), dict(lo=None, hi=dict(depth=1)), dict(lo=dict(albedo=1, normal=1), hi=dict(albedo=1)),
          dict(lo=dict(normal=1), hi={})], "one size only"),
        ([dict(lo=dict(albedo=0), hi=dict(albedo=1)), dict(lo=dict(depth=1), hi=dict(depth=0)),
          dict(lo=dict(albedo=1, normal=0, depth=1), hi=dict(albedo=1, normal=1, depth=1))], "guide has 0 samples"),
        ([dict(sigma_depth=0.0), dict(sigma_depth=-0.1), dict(sigma_depth=NAN), dict(sigma_depth=INF)], ".sigma_depth must"),
        ([dict(sigma_albedo=0.0), dict(sigma_albedo=-0.1), dict(sigma_albedo=NAN), dict(sigma_albedo=INF)], ".sigma_albedo must"),
        ([dict(normal_squarings=7), dict(normal_squarings=0xffffffff)], ".normal_squarings"),
        ([dict(min_weight=0.0), dict(min_weight=1.0), dict(min_weight=-0.5), dict(min_weight=NAN), dict(min_weight=INF)], ".min_weight must"),
        ([dict(max_value=0.0), dict(max_value=-1.0), dict(max_value=NAN), dict(max_value=INF)], ".max_value must"),
    ]
    for k, (cases, word) in enumerate(rules):
        for case in cases:
            kw = dict(case)
            rc, msg = _call(bendy, kw.pop("g", g), **kw)
            assert rc == -1 and word in msg, (case, msg)
            for later, _ in rules[k + 1:]:
                for other in later:
                    merged = {**other, **case}
                    rc, msg = _call(bendy, merged.pop("g", g), **merged)
                    assert rc == -1 and word in msg, (case, other, msg)
    st = bendy.UpscaleStats()
    assert lib.bt_upscale_poll(g, C.byref(st)) == -1             # a refused call is no call
    lib.bt_upscale_free(g)


def test_host_entry_point_refuses_the_same(bendy):
    ones = np.ones((4, 4, 4), dtype=np.float32)
    for kw, word in ((dict(width=3, height=8), "bt_resample"), (dict(width=8, height=3), "bt_resample"),
                     (dict(width=8, height=8, lo=(ones, None, None)), "one size only"),
                     (dict(width=8, height=8, lo=((ones, 0), None, None), hi=(np.ones((8, 8, 4), dtype=np.float32), None, None)), "0 samples"),
                     (dict(width=8, height=8, min_weight=1.5), ".min_weight"), (dict(width=8, height=8, samples=0), "0 samples")):
        kw = dict(kw)
        with pytest.raises(bendy.BendyError) as e:
            bendy.upscale_host(ones, kw.pop("samples", 1), kw.pop("width"), kw.pop("height"), **kw)
        assert e.value.code == -1 and word in str(e.value), (kw, str(e.value))


def test_valid_call_fails_loudly_without_gpu(bendy):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    g = C.c_void_p(bendy.api.lib.bt_upscale_new())
    both = dict(lo=dict(albedo=1, normal=4, depth=1), hi=dict(albedo=4, normal=1, depth=2))
    for kw in (dict(), dict(params={}), both, dict(lo={}, hi={}), dict(lo=dict(normal=1), hi=dict(normal=1)), dict(W=8, H=8), dict(W=8), dict(H=8),
               dict(w=1, h=1, W=1, H=1), dict(w=1, h=1, W=0x7fffffff, H=1),
               dict(sigma_depth=1e-30, sigma_albedo=3e38, normal_squarings=0, min_weight=1e-30, max_value=3e38),     # the ends of every range
               dict(sigma_depth=3e38, sigma_albedo=1e-30, normal_squarings=6, min_weight=0.999, max_value=1e-30)):
        rc, msg = _call(bendy, g, **kw)
        assert rc == -8, (kw, msg)                                   # BT_ERR_DEVICE, as bt_glare_device
    st = bendy.UpscaleStats()
    assert bendy.api.lib.bt_upscale_poll(g, C.byref(st)) == -1       # a failed call left no counts
    bendy.api.lib.bt_upscale_free(g)
