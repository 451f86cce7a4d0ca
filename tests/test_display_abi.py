"""The display stage (EXTENSION) on a machine without a GPU: the defaults, the handle's life cycle, what
bt_display_device refuses before it touches the device and in which order, and BT_ERR_DEVICE for a valid call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FAKE = [0x10000, 0x20000]          # never dereferenced: every call below fails before the device is touched
NAMES = ["bt_display_params_default", "bt_display_new", "bt_display_free", "bt_display_reset", "bt_display_device",
         "bt_display_exposure", "bt_debug_display_histogram", "bt_write_pfm"]
GOOD = dict(key=0.18, tonemap=2, auto_exposure=1, ev=0.0, p_low=0.10, p_high=0.02, adapt=1.0, ev_min=-8.0, ev_max=8.0, white=4.0)
NAN, INF = float("nan"), float("inf")


def _call(bendy, d, src=FAKE[0], samples=1, dst=FAKE[1], w=8, h=8, cs=3, params=None, **fields):
    lib = bendy.api.lib
    p = None
    if params is not None or fields:
        p = C.byref(bendy.api._CDisplayParams(*{**GOOD, **(params or {}), **fields}.values()))
    rc = lib.bt_display_device(d, src, samples, dst, w, h, cs, p, None)
    return rc, lib.bt_last_error().decode()


def test_symbols_and_defaults(bendy):
    api = bendy.api
    hdr = open(os.path.join(ROOT, "include", "bendy_hip.h")).read()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(api.lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    p = api._CDisplayParams()
    api.lib.bt_display_params_default(C.byref(p))
    api.lib.bt_display_params_default(None)
    got = {k: getattr(p, k) for k, _ in api._CDisplayParams._fields_}
    assert got == {k: (v if isinstance(v, int) or k == "key" else float(np.float32(v))) for k, v in GOOD.items()}
    assert C.sizeof(api._CDisplayParams) == 48
    assert (int(bendy.Tonemap.Clip), int(bendy.Tonemap.Reinhard), int(bendy.Tonemap.Aces)) == (0, 1, 2)
    q = bendy.DisplayParams(tonemap="reinhard", white=2)
    assert (q.tonemap, q.white, q.key, q.adapt) == (bendy.Tonemap.Reinhard, 2, p.key, 1.0)
    assert q._c().tonemap == 1 and q._c().white == 2.0


def test_new_reset_free_without_a_device(bendy):
    lib = bendy.api.lib
    d = C.c_void_p(lib.bt_display_new())
    assert d
    assert lib.bt_display_reset(d) == 0
    ev, mult = C.c_float(7.0), C.c_float(7.0)
    assert lib.bt_display_exposure(d, C.byref(ev), C.byref(mult)) == -1 and "no frame" in lib.bt_last_error().decode()
    assert (ev.value, mult.value) == (7.0, 7.0)
    assert lib.bt_debug_display_histogram(d, None, 0) == 258
    host = np.ones(300, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    assert lib.bt_debug_display_histogram(d, host.ctypes.data_as(u32p), 300) == 258 and not host[:258].any() and host[258:].all()
    assert lib.bt_debug_display_histogram(d, host.ctypes.data_as(u32p), 5) == 5
    assert lib.bt_debug_display_histogram(d, None, 5) == -1
    lib.bt_display_free(d)
    lib.bt_display_free(None)
    assert lib.bt_display_reset(None) == -1 and lib.bt_display_exposure(None, None, None) == -1
    assert lib.bt_debug_display_histogram(None, None, 0) == -1
    h = bendy.Display(tonemap="clip", adapt=0.5)
    assert h.params.tonemap == bendy.Tonemap.Clip and h.params.adapt == 0.5
    bins, under, over = h.histogram()
    assert bins.shape == (256,) and bins.dtype == np.uint32 and not bins.any() and (under, over) == (0, 0)
    with pytest.raises(bendy.BendyError) as e:
        h.exposure()
    assert e.value.code == -1
    h.reset()
    h.close()
    h.close()
    with pytest.raises(bendy.BendyError) as e:
        bendy.Display().present(bendy.Buffer(4, 4, device="cpu"))
    assert e.value.code == -1 and "host-buffer" in str(e.value)


def test_validation_order(bendy):
    """Each rule alone, and each rule together with a violation of every later one: the earlier rule's message wins."""
    lib = bendy.api.lib
    d = C.c_void_p(lib.bt_display_new())
    # (arguments that break the rule, a word of its message), in the header's order
    rules = [
        ([dict(d=None), dict(src=None), dict(dst=None)], "null"),
        ([dict(samples=0)], "0 samples"),
        ([dict(w=0), dict(h=0), dict(w=1 << 16, h=1 << 16)], "zero-sized"),
        ([dict(dst=FAKE[0])], "alias"),
        ([dict(cs=1), dict(cs=4), dict(cs=-1)], "colour space"),
        ([dict(tonemap=3), dict(tonemap=-1)], "tonemap"),
        ([dict(ev=NAN), dict(ev=INF), dict(ev=-INF)], ".ev must"),
        ([dict(key=0.0), dict(key=-1.0), dict(key=NAN), dict(key=INF)], ".key must"),
        ([dict(p_low=-0.01), dict(p_low=1.0), dict(p_high=-0.01), dict(p_high=1.0), dict(p_low=0.5, p_high=0.5), dict(p_low=NAN),
          dict(p_high=NAN)], "p_low and p_high"),
        ([dict(adapt=0.0), dict(adapt=-0.5), dict(adapt=1.5), dict(adapt=NAN)], ".adapt must"),
        ([dict(ev_min=1.0, ev_max=0.5), dict(ev_min=NAN), dict(ev_max=NAN)], "ev_min must"),
        ([dict(white=0.0), dict(white=-1.0), dict(white=NAN)], ".white must"),
    ]
    for k, (cases, word) in enumerate(rules):
        for case in cases:
            kw = dict(case)
            rc, msg = _call(bendy, kw.pop("d", d), **kw)
            assert rc == -1 and word in msg, (case, msg)
            for later, _ in rules[k + 1:]:
                merged = {**later[0], **case}
                rc, msg = _call(bendy, merged.pop("d", d), **merged)
                assert rc == -1 and word in msg, (case, later[0], msg)
    lib.bt_display_free(d)


def test_valid_call_fails_loudly_without_gpu(bendy):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    d = C.c_void_p(bendy.api.lib.bt_display_new())
    for kw in (dict(), dict(params={}), dict(cs=0), dict(cs=2), dict(tonemap=0, auto_exposure=0, ev=-3.5),
               dict(p_low=0.0, p_high=0.0, adapt=1.0, ev_min=2.0, ev_max=2.0, white=1e-3, tonemap=1),     # the ends of every range
               dict(adapt=1e-6, p_low=0.99, p_high=0.0, ev_min=-INF, ev_max=INF)):
        rc, msg = _call(bendy, d, **kw)
        assert rc == -8, (kw, msg)                                   # BT_ERR_DEVICE, as bt_denoise_device
    assert bendy.api.lib.bt_display_exposure(d, None, None) == -1    # a failed call displayed nothing
    bendy.api.lib.bt_display_free(d)
