"""The resample stage's own per-texel code and tables (csrc/bt_resample.hpp through bt_debug_resample_host and
bt_debug_resample_weights; EXTENSION) against the numpy restatement, bit for bit, on a machine without a GPU.  The
kernels of bt_resample.hip call the same functions."""
import numpy as np
import pytest

import resample_ref as r
from test_resample_ref import FILTERS, SHAPES

f32 = np.float32
SAMPLES = (1, 3)


def library_tables(handle):
    """Both tables of the handle's last call in axis_table's form."""
    return tuple((t[0].astype(np.int64), t[1], t[2], t[3].astype(np.int64)) for t in (handle.weights(0), handle.weights("y")))


def same_table(got, want, filt):
    """box, tent and mitchell are float64 + - * / alone: equal.  lanczos3 takes two sines, and two correct sines may differ in the
    last float64 bit, which can move a weight's float32 rounding by one ulp and no more."""
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2].shape == want[2].shape and np.array_equal(got[3], want[3])
    if filt != r.LANCZOS3:
        assert np.array_equal(got[2], want[2])
    else:
        assert (np.abs(got[2].astype(np.float64) - want[2].astype(np.float64)) <= np.spacing(np.abs(want[2])).astype(np.float64)).all()
        assert np.array_equal(got[2] == 0, want[2] == 0)                          # the exact zeros are exact on both sides


@pytest.mark.parametrize("src,dst", SHAPES)
def test_host_entry_point_is_the_restatement(bendy, src, dst):
    (w, h), (W, H) = src, dst
    frame = r.make_frame(w, h, seed=w * 1000 + h)
    assert w * h < 4 or not np.isfinite(frame[..., :3]).all()
    for filt in FILTERS:
        handle = bendy.Resample(filter=filt)
        for n in SAMPLES:
            for extra in (dict(), dict(clamp_negative=0), dict(max_value=0.5)):
                got = handle.host(frame, n, W, H, **extra)
                tables = library_tables(handle)
                want = r.resample(frame, n, W, H, **{**r.DEFAULTS, "filter": filt, **extra, "tables": tables})
                assert got.shape == (H, W, 4) and np.isfinite(got).all()
                assert np.array_equal(got, want), (filt, n, extra, np.argwhere(got != want)[:4])        # no pixel is exempt
        same_table(tables[0], r.axis_table(w, W, filt), filt)
        same_table(tables[1], r.axis_table(h, H, filt), filt)
        # without a handle the entry point builds the same tables
        assert np.array_equal(bendy.resample_host(frame, 3, W, H, filter=filt), handle.host(frame, 3, W, H))
        handle.close()


def test_filters_by_name_and_defaults(bendy):
    frame = r.make_frame(16, 17, seed=5)
    assert [int(f) for f in bendy.Filter] == [0, 1, 2, 3] and [f.name.lower() for f in bendy.Filter] == list(r.FILTERS)
    want = r.resample(frame, 2, 7, 9, **r.DEFAULTS)
    assert np.array_equal(bendy.resample_host(frame, 2, 7, 9), want)
    assert np.array_equal(bendy.resample_host(frame, 2, 7, 9, filter="mitchell"), want)
    assert np.array_equal(bendy.resample_host(frame, 2, 7, 9, filter=bendy.Filter.Lanczos3), r.resample(frame, 2, 7, 9, filter=r.LANCZOS3))
    with pytest.raises(bendy.BendyError):
        bendy.ResampleParams(filter="bicubic")


def test_a_handle_keeps_and_replaces_its_tables(bendy):
    handle = bendy.Resample(filter="tent")
    with pytest.raises(bendy.BendyError):
        handle.weights(0)                                                          # no call yet
    frame = r.make_frame(45, 35, seed=1)
    handle.host(frame, 1, 16, 17)
    a = library_tables(handle)
    handle.host(frame, 1, 16, 17, filter="box")
    b = library_tables(handle)
    assert (a[0][1], a[1][1]) == (r.axis_table(45, 16, r.TENT)[1], r.axis_table(35, 17, r.TENT)[1])
    assert (b[0][1], b[1][1]) == (r.axis_table(45, 16, r.BOX)[1], r.axis_table(35, 17, r.BOX)[1]) and b[0][1] < a[0][1]
    handle.host(r.make_frame(16, 17, seed=2), 1, 45, 35)
    assert library_tables(handle)[0][2].shape == (45, r.axis_table(16, 45, r.TENT)[1])
    handle.host(frame, 1, 16, 17)
    same_table(library_tables(handle)[0], a[0], r.TENT)
    with pytest.raises(bendy.BendyError):
        handle.weights(2)


def test_host_entry_point_validates(bendy):
    frame = r.make_frame(4, 4, poison=False)
    for bad in (dict(filter=4), dict(filter=-1), dict(max_value=0.0), dict(max_value=float("inf")), dict(max_value=float("nan"))):
        with pytest.raises(bendy.BendyError) as e:
            bendy.resample_host(frame, 1, 3, 3, **bad)
        assert e.value.code == -1, bad
    for args in ((0, 3, 3), (1, 0, 3), (1, 3, 0)):
        with pytest.raises(bendy.BendyError):
            bendy.resample_host(frame, *args)
    with pytest.raises(bendy.BendyError):
        bendy.resample_host(frame[..., :3], 1, 3, 3)
    with pytest.raises(bendy.BendyError) as e:
        bendy.resample_host(r.make_frame(300, 2, poison=False), 1, 2, 2, filter="lanczos3")      # 150 : 1
    assert "x axis" in str(e.value) and "150" in str(e.value)
