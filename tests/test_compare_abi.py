"""The compare stage (EXTENSION) on a machine without a GPU: the defaults, the handle's life cycle, what
bt_compare_device refuses before it touches the device and in which order, BT_ERR_DEVICE for a valid call, and bt_read_pfm."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT

FAKE = [0x10000, 0x20000, 0x30000]      # never dereferenced: every call fails before the device
NAMES = ["bt_compare_params_default", "bt_compare_new", "bt_compare_free", "bt_compare_device", "bt_compare_poll", "bt_compare_tail",
         "bt_compare_map_device", "bt_debug_compare_plane", "bt_debug_compare_host", "bt_read_pfm"]
NAN, INF = float("nan"), float("inf")
NO_PARAMS = object()


def _call(bendy, g, test=FAKE[0], ns=1, ref=FAKE[1], nr=1, w=8, h=8, params=None, epsilon=0.01, peak=1.0):
    lib = bendy.api.lib
    p = None if params is NO_PARAMS else C.byref(bendy.api._CCompareParams(epsilon, peak))
    rc = lib.bt_compare_device(g, test, ns, ref, nr, w, h, p, None)
    return rc, lib.bt_last_error().decode()


def test_symbols_and_defaults(bendy):
    api = bendy.api
    hdr = open(os.path.join(ROOT, "include", "bendy_hip.h")).read()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(api.lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    for name in ("bt_compare_params", "bt_compare_stats", "bt_compare"):
        assert re.search(r"\}\s*%s;|typedef struct %s %s;" % (name, name, name), hdr), name
    p = api._CCompareParams()
    api.lib.bt_compare_params_default(C.byref(p))
    api.lib.bt_compare_params_default(None)
    assert (p.epsilon, p.peak) == (0.01, 1.0)
    assert C.sizeof(api._CCompareParams) == 16 and C.sizeof(api.CompareStats) == 72
    q = bendy.CompareParams(peak=2.0)
    assert (q.epsilon, q.peak) == (0.01, 2.0) and q._c().peak == 2.0
    hpp = open(os.path.join(ROOT, "include", "bendy_tracer.hpp")).read()
    assert "class Compare" in hpp and "bt_compare_device(h_" in hpp


def test_new_free_and_calls_before_any_measure(bendy):
    lib = bendy.api.lib
    g = C.c_void_p(lib.bt_compare_new())
    assert g
    st, share, thr = bendy.CompareStats(), C.c_double(), C.c_float()
    assert lib.bt_compare_poll(g, C.byref(st)) == -1 and "before" in lib.bt_last_error().decode()
    assert lib.bt_compare_poll(g, None) == -1 and lib.bt_compare_poll(None, C.byref(st)) == -1
    assert lib.bt_compare_tail(g, 0.01, C.byref(share), C.byref(thr)) == -1 and "before" in lib.bt_last_error().decode()
    for f in (0.0, -0.5, 1.5, NAN, INF):
        assert lib.bt_compare_tail(g, f, C.byref(share), C.byref(thr)) == -1 and "fraction" in lib.bt_last_error().decode(), f
    assert lib.bt_compare_tail(None, 0.01, None, None) == -1
    assert lib.bt_compare_map_device(g, FAKE[2], 1.0, None) == -1 and "before" in lib.bt_last_error().decode()
    for s in (0.0, -1.0, NAN, INF):
        assert lib.bt_compare_map_device(g, FAKE[2], s, None) == -1 and "scale" in lib.bt_last_error().decode(), s
    assert lib.bt_compare_map_device(g, None, 1.0, None) == -1 and lib.bt_compare_map_device(None, FAKE[2], 1.0, None) == -1
    assert lib.bt_debug_compare_plane(g, 0, None, 0) == -1 and lib.bt_debug_compare_plane(g, 3, None, 0) == -1
    assert lib.bt_debug_compare_plane(None, 0, None, 0) == -1
    lib.bt_compare_free(g)
    lib.bt_compare_free(None)
    h = bendy.Compare(epsilon=1e-4)
    assert (h.params.epsilon, h.params.peak) == (1e-4, 1.0)
    for call in (h.poll, h.tail, h.map, lambda: h.plane(0)):
        with pytest.raises(bendy.BendyError) as e:
            call()
        assert e.value.code == -1
    with pytest.raises(bendy.BendyError) as e:
        h.measure(bendy.Buffer(4, 4, device="cpu"), bendy.Buffer(4, 4, device="cpu"))
    assert e.value.code == -1 and "host-buffer" in str(e.value)
    h.close()
    h.close()


def test_validation_order(bendy):
    """Each rule alone, and each rule together with a violation of every later one: the earlier rule's message wins."""
    lib = bendy.api.lib
    g = C.c_void_p(lib.bt_compare_new())
    rules = [
        ([dict(g=None), dict(test=None), dict(ref=None), dict(params=NO_PARAMS)], "null"),
        ([dict(ns=0), dict(nr=0), dict(ns=0, nr=0)], "0 samples"),
        ([dict(w=0), dict(h=0), dict(w=1 << 16, h=1 << 16), dict(w=1 << 31, h=1), dict(w=1, h=1 << 31)], "zero-sized"),
        ([dict(epsilon=0.0), dict(epsilon=-0.01), dict(epsilon=NAN), dict(epsilon=INF)], ".epsilon must"),
        ([dict(peak=0.0), dict(peak=-1.0), dict(peak=NAN), dict(peak=INF)], ".peak must"),
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
    st = bendy.CompareStats()
    assert lib.bt_compare_poll(g, C.byref(st)) == -1             # a refused call is no call
    lib.bt_compare_free(g)


def test_valid_call_fails_loudly_without_gpu(bendy):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    g = C.c_void_p(bendy.api.lib.bt_compare_new())
    for kw in (dict(), dict(ref=FAKE[0]), dict(ns=3, nr=4), dict(w=1, h=1), dict(w=0x7fffffff, h=1), dict(w=1, h=0x7fffffff),
               dict(w=0xffff, h=0x10001), dict(epsilon=1e-300, peak=1e300), dict(epsilon=1e300, peak=1e-300)):
        rc, msg = _call(bendy, g, **kw)
        assert rc == -8, (kw, msg)                                   # BT_ERR_DEVICE
    st = bendy.CompareStats()
    assert bendy.api.lib.bt_compare_poll(g, C.byref(st)) == -1       # a failed call left no results
    bendy.api.lib.bt_compare_free(g)


# ---- bt_read_pfm ----
def _read(bendy, path, capacity=None):
    lib = bendy.api.lib
    w, h = C.c_uint32(0), C.c_uint32(0)
    rc = lib.bt_read_pfm(os.fsencode(str(path)), None, 0, C.byref(w), C.byref(h))
    if rc or capacity == 0:
        return rc, None, w.value, h.value
    a = np.full(w.value * h.value * 4 if capacity is None else capacity, -7.0, dtype=np.float32)
    rc = lib.bt_read_pfm(os.fsencode(str(path)), a.ctypes.data_as(C.POINTER(C.c_float)), a.size, C.byref(w), C.byref(h))
    return rc, a, w.value, h.value


def test_pfm_round_trip_is_bit_for_bit(bendy, tmp_path):
    rng = np.random.default_rng(1)
    for w, h, samples in ((1, 1, 1), (5, 3, 1), (45, 35, 3), (64, 36, 4)):
        frame = np.exp2(rng.uniform(-20, 20, size=(h, w, 4))).astype(np.float32) * np.float32(samples)
        frame[0, 0, 0], frame[-1, -1, 2] = -0.0, np.inf
        path = tmp_path / f"f{w}.pfm"
        bendy.write_pfm(path, frame, samples)
        got, gw, gh = bendy.read_pfm(path)
        want = frame[..., :3] * (np.float32(1.0) / np.float32(samples))
        assert (gw, gh) == (w, h) and got.shape == (h, w, 4) and (got[..., 3] == 1.0).all()
        assert np.array_equal(got[..., :3].view(np.uint32), want.view(np.uint32))         # rows top-down again, every bit
        assert _read(bendy, path, capacity=0)[2:] == (w, h)                                # the size-only call


def _pfm(path, magic, w, h, scale, rows_bottom_up, order):
    with open(path, "wb") as f:
        f.write(f"{magic}\n{w} {h}\n{scale}\n".encode())
        f.write(np.ascontiguousarray(rows_bottom_up, dtype=order + "f4").tobytes())
    return path


def test_pfm_byte_orders_and_grey(bendy, tmp_path):
    rgb = np.arange(2 * 3 * 3, dtype=np.float32).reshape(2, 3, 3) + 0.25           # top-down
    for scale, order in (("-1.0", "<"), ("-2.5", "<"), ("1.0", ">"), ("255", ">")):    # the magnitude is ignored
        got, w, h = bendy.read_pfm(_pfm(tmp_path / "c.pfm", "PF", 3, 2, scale, rgb[::-1], order))
        assert (w, h) == (3, 2) and np.array_equal(got[..., :3], rgb) and (got[..., 3] == 1.0).all(), scale
    grey = np.arange(6, dtype=np.float32).reshape(2, 3) - 1.5
    for scale, order in (("-1.0", "<"), ("1.0", ">")):
        got, w, h = bendy.read_pfm(_pfm(tmp_path / "g.pfm", "Pf", 3, 2, scale, grey[::-1], order))
        assert (w, h) == (3, 2) and all(np.array_equal(got[..., k], grey) for k in range(3)) and (got[..., 3] == 1.0).all()


def test_pfm_errors(bendy, tmp_path):
    lib = bendy.api.lib
    assert _read(bendy, tmp_path / "missing.pfm")[0] == -2                               # BT_ERR_IO
    good = _pfm(tmp_path / "ok.pfm", "PF", 3, 2, "-1.0", np.zeros((2, 3, 3)), "<")
    data = open(good, "rb").read()
    bad = {"truncated data": data[:-1], "truncated header": b"PF\n3 2\n", "empty": b"", "magic": b"P6" + data[2:], "no scale": b"PF\n3 2\n\n" + data[11:],
           "zero scale": b"PF\n3 2\n0.0\n" + data[12:], "zero side": b"PF\n0 2\n-1.0\n", "negative side": b"PF\n-3 2\n-1.0\n" + data[12:],
           "words": b"PF\nthree 2\n-1.0\n" + data[12:], "huge": b"PF\n70000 70000\n-1.0\n", "long token": b"PF\n" + b"1" * 64 + b" 2\n-1.0\n"}
    for what, blob in bad.items():
        p = tmp_path / "bad.pfm"
        p.write_bytes(blob)
        rc = _read(bendy, p)[0]
        assert rc == -3, (what, rc, lib.bt_last_error().decode())                       # BT_ERR_PARSE
    rc, a, w, h = _read(bendy, good, capacity=23)
    assert rc == -1 and "24" in lib.bt_last_error().decode() and (a == -7.0).all()       # too small a buffer is left alone
    w_, h_ = C.c_uint32(), C.c_uint32()
    assert lib.bt_read_pfm(None, None, 0, C.byref(w_), C.byref(h_)) == -1 and lib.bt_read_pfm(os.fsencode(str(good)), None, 0, None, C.byref(h_)) == -1
    with pytest.raises(bendy.BendyError) as e:
        bendy.read_pfm(tmp_path / "missing.pfm")
    assert e.value.code == -2
