"""The despeckle stage (EXTENSION) on a machine without a GPU: the defaults, the handle's life cycle, what
bt_despeckle_device refuses before it touches the device and in which order, and BT_ERR_DEVICE for a valid call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FAKE = [0x10000, 0x20000]          # never dereferenced: every call below fails before the device is touched
NAMES = ["bt_despeckle_params_default", "bt_despeckle_new", "bt_despeckle_free", "bt_despeckle_device", "bt_despeckle_poll",
         "bt_debug_despeckle_host"]
GOOD = dict(radius=1, rank=2, ratio=4.0, floor=0.01, max_value=65536.0)
NAN, INF = float("nan"), float("inf")


def _call(bendy, g, src=FAKE[0], samples=1, dst=FAKE[1], w=8, h=8, params=None, **fields):
    lib = bendy.api.lib
    p = None
    if params is not None or fields:
        p = C.byref(bendy.api._CDespeckleParams(*{**GOOD, **(params or {}), **fields}.values()))
    rc = lib.bt_despeckle_device(g, src, samples, dst, w, h, p, None)
    return rc, lib.bt_last_error().decode()


def test_symbols_and_defaults(bendy):
    api = bendy.api
    hdr = open(os.path.join(ROOT, "include", "bendy_hip.h")).read()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(api.lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    for name in ("bt_despeckle_params", "bt_despeckle_stats", "bt_despeckle"):
        assert re.search(r"\}\s*%s;|typedef struct %s %s;" % (name, name, name), hdr), name
    p = api._CDespeckleParams()
    api.lib.bt_despeckle_params_default(C.byref(p))
    api.lib.bt_despeckle_params_default(None)
    got = {k: getattr(p, k) for k, _ in api._CDespeckleParams._fields_}
    assert got == {k: (v if isinstance(v, int) else float(np.float32(v))) for k, v in GOOD.items()}
    assert C.sizeof(api._CDespeckleParams) == 20 and C.sizeof(api.DespeckleStats) == 16
    q = bendy.DespeckleParams(rank=3, ratio=8.0)
    assert (q.radius, q.rank, q.ratio, q.floor, q.max_value) == (1, 3, 8.0, float(np.float32(0.01)), 65536.0)
    assert q._c().rank == 3 and q._c().ratio == 8.0
    # the C++ delegate is declared next to the others
    hpp = open(os.path.join(ROOT, "include", "bendy_tracer.hpp")).read()
    assert "class Despeckle" in hpp and "bt_despeckle_device(h_" in hpp


def test_new_free_and_poll_without_a_device(bendy):
    lib = bendy.api.lib
    g = C.c_void_p(lib.bt_despeckle_new())
    assert g
    st = bendy.DespeckleStats()
    assert lib.bt_despeckle_poll(g, C.byref(st)) == -1 and "before" in lib.bt_last_error().decode()      # no call yet
    assert lib.bt_despeckle_poll(g, None) == -1 and lib.bt_despeckle_poll(None, C.byref(st)) == -1
    lib.bt_despeckle_free(g)
    lib.bt_despeckle_free(None)
    h = bendy.Despeckle(radius=2, ratio=2.0)
    assert (h.params.radius, h.params.rank, h.params.ratio, h.params.floor) == (2, 2, 2.0, float(np.float32(0.01)))
    with pytest.raises(bendy.BendyError) as e:
        h.poll()
    assert e.value.code == -1
    with pytest.raises(bendy.BendyError) as e:
        h.apply(bendy.Buffer(4, 4, device="cpu"))
    assert e.value.code == -1 and "host-buffer" in str(e.value)
    h.close()
    h.close()


def test_validation_order(bendy):
    """Each rule alone, and each rule together with a violation of every later one: the earlier rule's message wins."""
    lib = bendy.api.lib
    g = C.c_void_p(lib.bt_despeckle_new())
    # (arguments that break the rule, a word of its message), in the header's order
    rules = [
        ([dict(g=None), dict(src=None), dict(dst=None)], "null"),
        ([dict(samples=0)], "0 samples"),
        ([dict(w=0), dict(h=0), dict(w=1 << 16, h=1 << 16)], "zero-sized"),
        ([dict(dst=FAKE[0])], "alias"),
        ([dict(radius=0), dict(radius=3), dict(radius=0xffffffff)], ".radius"),
        ([dict(rank=0), dict(rank=9), dict(radius=2, rank=25), dict(rank=0xffffffff)], ".rank"),
        ([dict(ratio=0.999), dict(ratio=0.0), dict(ratio=-4.0), dict(ratio=NAN), dict(ratio=INF)], ".ratio must"),
        ([dict(floor=-1e-6), dict(floor=NAN), dict(floor=INF)], ".floor must"),
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
    st = bendy.DespeckleStats()
    assert lib.bt_despeckle_poll(g, C.byref(st)) == -1          # a refused call is no call
    lib.bt_despeckle_free(g)


def test_valid_call_fails_loudly_without_gpu(bendy):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    g = C.c_void_p(bendy.api.lib.bt_despeckle_new())
    for kw in (dict(), dict(params={}), dict(radius=1, rank=8), dict(radius=2, rank=24, ratio=1.0, floor=0.0, max_value=3e38),     # the ends of every range
               dict(radius=2, rank=1, ratio=3e38, floor=3e38, max_value=1e-30), dict(w=1, h=1), dict(w=0xffffffff, h=1)):
        rc, msg = _call(bendy, g, **kw)
        assert rc == -8, (kw, msg)                                   # BT_ERR_DEVICE, as bt_glare_device
    st = bendy.DespeckleStats()
    assert bendy.api.lib.bt_despeckle_poll(g, C.byref(st)) == -1     # a failed call left no counts
    bendy.api.lib.bt_despeckle_free(g)
