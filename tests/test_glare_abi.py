"""The glare stage (EXTENSION) on a machine without a GPU: the defaults, the handle's life cycle, what
bt_glare_device refuses before it touches the device and in which order, and BT_ERR_DEVICE for a valid call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FAKE = [0x10000, 0x20000]          # never dereferenced: every call below fails before the device is touched
NAMES = ["bt_glare_params_default", "bt_glare_new", "bt_glare_free", "bt_glare_device", "bt_debug_glare_plane", "bt_debug_glare_host"]
GOOD = dict(levels=6, spread=1.0, strength=0.08, max_value=65536.0)
NAN, INF = float("nan"), float("inf")


def _call(bendy, g, src=FAKE[0], samples=1, dst=FAKE[1], w=8, h=8, params=None, **fields):
    lib = bendy.api.lib
    p = None
    if params is not None or fields:
        p = C.byref(bendy.api._CGlareParams(*{**GOOD, **(params or {}), **fields}.values()))
    rc = lib.bt_glare_device(g, src, samples, dst, w, h, p, None)
    return rc, lib.bt_last_error().decode()


def test_symbols_and_defaults(bendy):
    api = bendy.api
    hdr = open(os.path.join(ROOT, "include", "bendy_hip.h")).read()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(api.lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    p = api._CGlareParams()
    api.lib.bt_glare_params_default(C.byref(p))
    api.lib.bt_glare_params_default(None)
    got = {k: getattr(p, k) for k, _ in api._CGlareParams._fields_}
    assert got == {k: (v if isinstance(v, int) else float(np.float32(v))) for k, v in GOOD.items()}
    assert C.sizeof(api._CGlareParams) == 16
    q = bendy.GlareParams(levels=3, strength=0.5)
    assert (q.levels, q.strength, q.spread, q.max_value) == (3, 0.5, 1.0, 65536.0)
    assert q._c().levels == 3 and q._c().strength == 0.5


def test_new_free_and_planes_without_a_device(bendy):
    lib = bendy.api.lib
    g = C.c_void_p(lib.bt_glare_new())
    assert g
    for level in (0, 1, 16, 17):                         # no call yet: there is no plane
        assert lib.bt_debug_glare_plane(g, level, None, 0) == -1 and "level" in lib.bt_last_error().decode()
    lib.bt_glare_free(g)
    lib.bt_glare_free(None)
    assert lib.bt_debug_glare_plane(None, 1, None, 0) == -1
    h = bendy.Glare(levels=2, spread=2.0)
    assert (h.params.levels, h.params.spread, h.params.strength) == (2, 2.0, float(np.float32(0.08)))
    with pytest.raises(bendy.BendyError) as e:
        h.plane(1)
    assert e.value.code == -1
    with pytest.raises(bendy.BendyError) as e:
        h.apply(bendy.Buffer(4, 4, device="cpu"))
    assert e.value.code == -1 and "host-buffer" in str(e.value)
    h.close()
    h.close()


def test_validation_order(bendy):
    """Each rule alone, and each rule together with a violation of every later one: the earlier rule's message wins."""
    lib = bendy.api.lib
    g = C.c_void_p(lib.bt_glare_new())
    # (arguments that break the rule, a word of its message), in the header's order
    rules = [
        ([dict(g=None), dict(src=None), dict(dst=None)], "null"),
        ([dict(samples=0)], "0 samples"),
        ([dict(w=0), dict(h=0), dict(w=1 << 16, h=1 << 16)], "zero-sized"),
        ([dict(dst=FAKE[0])], "alias"),
        ([dict(levels=17), dict(levels=0xffffffff)], ".levels"),
        ([dict(spread=0.0), dict(spread=-1.0), dict(spread=16.5), dict(spread=NAN), dict(spread=INF)], ".spread must"),
        ([dict(strength=-0.01), dict(strength=1.01), dict(strength=NAN), dict(strength=INF)], ".strength must"),
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
    lib.bt_glare_free(g)


def test_valid_call_fails_loudly_without_gpu(bendy):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    g = C.c_void_p(bendy.api.lib.bt_glare_new())
    for kw in (dict(), dict(params={}), dict(levels=0), dict(levels=16, spread=16.0, strength=1.0, max_value=3e38),     # the ends of every range
               dict(spread=1e-6, strength=0.0, max_value=1e-30), dict(w=1, h=1), dict(w=0xffffffff, h=1, levels=0)):
        rc, msg = _call(bendy, g, **kw)
        assert rc == -8, (kw, msg)                                   # BT_ERR_DEVICE, as bt_display_device
    assert bendy.api.lib.bt_debug_glare_plane(g, 1, None, 0) == -1   # a failed call left no plane
    bendy.api.lib.bt_glare_free(g)
