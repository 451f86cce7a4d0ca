"""bt_write_pfm / api.write_pfm (EXTENSION): the linear frame as a Portable Float Map, read back with numpy."""
import numpy as np
import pytest


def read_pfm(path):
    raw = open(path, "rb").read()
    magic, dims, scale, body = raw.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    return magic, scale, np.frombuffer(body, dtype="<f4").reshape(h, w, 3)


def test_write_pfm_round_trip(bendy, tmp_path):
    rng = np.random.default_rng(3)
    w, h, n = 5, 3, 3
    sums = rng.uniform(0.0, 60.0, size=(h, w, 4)).astype(np.float32)
    sums[1, 2, :3] = (0.0, 1e-30, 1e30)
    sums[..., 3] = 1.0
    path = tmp_path / "frame.pfm"
    bendy.write_pfm(path, sums, n)
    raw = open(path, "rb").read()
    assert raw.startswith(b"PF\n5 3\n-1.0\n") and len(raw) == len(b"PF\n5 3\n-1.0\n") + w * h * 12
    magic, scale, rows = read_pfm(path)
    assert (magic, scale) == (b"PF", b"-1.0")              # a negative scale: little-endian
    want = sums[..., :3] * (np.float32(1.0) / np.float32(n))
    assert np.array_equal(rows[::-1].view(np.uint32), want.view(np.uint32))       # rows bottom to top, values bit for bit
    assert not np.array_equal(rows, want)                                          # (the frame is not symmetric)
    bendy.write_pfm(path, sums)                                                    # samples = 1: the frame as it is
    assert np.array_equal(read_pfm(path)[2][::-1], sums[..., :3])


def test_write_pfm_errors(bendy, tmp_path):
    a = np.zeros((2, 2, 4), dtype=np.float32)
    with pytest.raises(bendy.BendyError) as e:
        bendy.write_pfm(tmp_path / "x.pfm", a, 0)
    assert e.value.code == -1
    with pytest.raises(bendy.BendyError) as e:
        bendy.write_pfm(tmp_path / "no_such_dir" / "x.pfm", a, 1)
    assert e.value.code == -2
    assert bendy.api.lib.bt_write_pfm(None, None, 1, 1, 1) == -1
