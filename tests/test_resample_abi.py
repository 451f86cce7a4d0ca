"""The resample stage (EXTENSION) on a machine without a GPU: the defaults, the handle's life cycle, what
bt_resample_device refuses before it touches the device and in which order, and BT_ERR_DEVICE for a valid call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FAKE = [0x10000, 0x20000]          # never dereferenced: every call below fails before the device is touched
NAMES = ["bt_resample_params_default", "bt_resample_new", "bt_resample_free", "bt_resample_device", "bt_debug_resample_weights",
         "bt_debug_resample_plane", "bt_debug_resample_host"]
GOOD = dict(filter=2, max_value=65536.0, clamp_negative=1)
NAN, INF = float("nan"), float("inf")


def _call(bendy, g, src=FAKE[0], samples=1, w=8, h=8, dst=FAKE[1], W=5, H=12, params=None, **fields):
    lib = bendy.api.lib
    p = None
    if params is not None or fields:
        p = C.byref(bendy.api._CResampleParams(*{**GOOD, **(params or {}), **fields}.values()))
    rc = lib.bt_resample_device(g, src, samples, w, h, dst, W, H, p, None)
    return rc, lib.bt_last_error().decode()


def test_symbols_and_defaults(bendy):
    api = bendy.api
    hdr = open(os.path.join(ROOT, "include", "bendy_hip.h")).read()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(api.lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    p = api._CResampleParams()
    api.lib.bt_resample_params_default(C.byref(p))
    api.lib.bt_resample_params_default(None)
    assert {k: getattr(p, k) for k, _ in api._CResampleParams._fields_} == GOOD
    assert C.sizeof(api._CResampleParams) == 12
    for name, value in (("BT_RESAMPLE_BOX", 0), ("BT_RESAMPLE_TENT", 1), ("BT_RESAMPLE_MITCHELL", 2), ("BT_RESAMPLE_LANCZOS3", 3)):
        assert re.search(r"\b%s = %d\b" % (name, value), hdr)
    q = bendy.ResampleParams(filter="lanczos3", clamp_negative=0)
    assert (q.filter, q.max_value, q.clamp_negative) == (bendy.Filter.Lanczos3, 65536.0, 0)
    assert q._c().filter == 3 and q._c().clamp_negative == 0
    tracer_hpp = open(os.path.join(ROOT, "include", "bendy_tracer.hpp")).read()
    assert "class Resample" in tracer_hpp and "bt_resample_device(h_" in tracer_hpp


def test_new_free_and_debug_calls_without_a_device(bendy):
    lib = bendy.api.lib
    g = C.c_void_p(lib.bt_resample_new())
    assert g
    assert lib.bt_debug_resample_plane(g, None, 0) == -1 and "no plane" in lib.bt_last_error().decode()       # no call yet
    for axis in (0, 1):
        assert lib.bt_debug_resample_weights(g, axis, None, None, None, None) == -1 and "no table" in lib.bt_last_error().decode()
    assert lib.bt_debug_resample_weights(g, 2, None, None, None, None) == -1 and "axis" in lib.bt_last_error().decode()
    lib.bt_resample_free(g)
    lib.bt_resample_free(None)
    assert lib.bt_debug_resample_plane(None, None, 0) == -1 and lib.bt_debug_resample_weights(None, 0, None, None, None, None) == -1
    h = bendy.Resample(filter="tent", max_value=2.0)
    assert (h.params.filter, h.params.max_value, h.params.clamp_negative) == (bendy.Filter.Tent, 2.0, 1)
    with pytest.raises(bendy.BendyError) as e:
        h.plane()
    assert e.value.code == -1
    with pytest.raises(bendy.BendyError) as e:
        h.apply(bendy.Buffer(4, 4, device="cpu"), 2, 2)
    assert e.value.code == -1 and "host-buffer" in str(e.value)
    h.close()
    h.close()


def test_validation_order(bendy):
    """Each rule alone, and each rule together with a violation of every later one: the earlier rule's message wins."""
    lib = bendy.api.lib
    g = C.c_void_p(lib.bt_resample_new())
    # (arguments that break the rule, a word of its message), in the header's order
    rules = [
        ([dict(g=None), dict(src=None), dict(dst=None)], "null"),
        ([dict(samples=0)], "0 samples"),
        ([dict(w=0), dict(h=0), dict(W=0), dict(H=0), dict(w=1 << 16, h=1 << 16), dict(W=1 << 16, H=1 << 16), dict(w=1 << 31, h=1),
          dict(W=1, H=1 << 31)], "zero-sized"),
        ([dict(dst=FAKE[0])], "alias"),
        ([dict(filter=4), dict(filter=-1), dict(filter=0x7fffffff)], ".filter"),
        ([dict(max_value=0.0), dict(max_value=-1.0), dict(max_value=NAN), dict(max_value=INF)], ".max_value must"),
        ([dict(w=4096, W=8), dict(w=129, W=1, filter=0)], "the x axis"),
        ([dict(h=4096, H=8), dict(h=2200, H=100, filter=3)], "the y axis"),
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
    lib.bt_resample_free(g)


def test_more_than_128_taps_is_refused_with_the_axis_and_the_ratio(bendy):
    lib = bendy.api.lib
    g = C.c_void_p(lib.bt_resample_new())
    # lanczos3 takes 6 s + 1 taps at a whole ratio s: 127 at 21 : 1 (c_i is whole), 132 at 22 : 1; box s (+ 1 where a tap falls on its edge)
    for kw, ok in ((dict(w=2100, W=100, filter=3), True), (dict(w=2200, W=100, filter=3), False), (dict(h=2200, H=100, filter=3), False),
                   (dict(w=3175, W=100, filter=2), True), (dict(w=3300, W=100, filter=2), False), (dict(w=6300, W=100, filter=1), True),
                   (dict(w=6500, W=100, filter=1), False), (dict(w=127, W=1, filter=0), True), (dict(w=12900, W=100, filter=0), False),
                   (dict(w=0x7fffffff, h=1, W=1, H=1, filter=0), False), (dict(w=8, W=0x7fffffff, H=1, filter=3), True)):
        rc, msg = _call(bendy, g, **kw)
        if ok:
            assert rc != -1, (kw, msg)
        else:
            axis = "x" if "w" in kw else "y"
            assert rc == -1 and "the %s axis" % axis in msg and "taps" in msg and "128" in msg, (kw, msg)
            if kw.get("w") == 2200 or kw.get("h") == 2200:
                assert "2200 -> 100" in msg and "ratio 22" in msg and "132 taps" in msg and "lanczos3" in msg, msg
    lib.bt_resample_free(g)


def test_valid_call_fails_loudly_without_gpu(bendy):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    g = C.c_void_p(bendy.api.lib.bt_resample_new())
    for kw in (dict(), dict(params={}), dict(filter=0), dict(filter=1), dict(filter=3, clamp_negative=0, max_value=3e38), dict(max_value=1e-30),
               dict(w=1, h=1, W=1, H=1), dict(w=1, h=1, W=5, H=3), dict(w=0x7fffffff, h=1, W=0x7fffffff, H=1), dict(w=2100, W=100, filter=3)):
        rc, msg = _call(bendy, g, **kw)
        assert rc == -8, (kw, msg)                                   # BT_ERR_DEVICE, as bt_glare_device
    assert bendy.api.lib.bt_debug_resample_plane(g, None, 0) == -1   # a failed call left no plane
    assert bendy.api.lib.bt_debug_resample_weights(g, 0, None, None, None, None) == -1          # and built no table
    bendy.api.lib.bt_resample_free(g)
