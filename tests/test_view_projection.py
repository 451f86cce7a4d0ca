"""bt_view's two maps (EXTENSION; csrc/bt_view.hpp through bt_debug_reproject) against a float64 restatement, on a
machine without a GPU.  The largest disagreement in pixels measured here is temporal_ref.EPS_PX; the bound is 4 x that value,
the margin covering asinf / atan2f / sinf / cosf differing between the host's and the device's maths library."""
import ctypes as C
import math

import numpy as np
import pytest

import temporal_ref as tr

FRAMES_ALL = [(1, 1), (16, 17), (45, 35), (64, 36)]          # every pixel
FRAMES_EDGE = [(768, 512), (3840, 2160)]                     # the border and the two diagonals
DEPTHS = [0.002, 0.3, 1.0]                                   # 0 < z < 1 (t = 2 and 300 scene units) and z = 1 (at infinity)


def rot(axis, a):
    x, y, z = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    c, s = math.cos(a), math.sin(a)
    return np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                     [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                     [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])


def make_view(bendy, L, T, w, h, n, yfov=0.6):
    v = bendy.View()
    m = np.concatenate([np.asarray(L, dtype=np.float64).T.reshape(-1), np.asarray(T, dtype=np.float64)]).astype(np.float32)
    v.to_world = (C.c_float * 12)(*[float(a) for a in m])
    v.yfov = yfov
    v.xfov = float(np.float32(v.yfov) * np.float32(w / h))
    v.clip_min, v.clip_max = 0.01, 1000.0
    v.width, v.height, v.subsample_n = w, h, n
    return v


BASE_L, BASE_T = rot([0.2, 1.0, 0.1], 0.7), np.array([1.5, -0.75, 4.0])


def pose_pairs(bendy, w, h, n):
    """(name, cur, prev): identical up to one ulp of one matrix entry; a pure yaw; a translation plus a rotation."""
    cur = make_view(bendy, BASE_L, BASE_T, w, h, n)
    ulp = make_view(bendy, BASE_L, BASE_T, w, h, n)
    ulp.to_world[4] = float(np.nextafter(np.float32(ulp.to_world[4]), np.float32(2.0)))
    yaw = make_view(bendy, BASE_L @ rot([0, 1, 0], 0.03), BASE_T, w, h, n)
    both = make_view(bendy, BASE_L @ rot([0.3, 1.0, -0.2], 0.02), BASE_T + np.array([0.05, -0.02, 0.03]), w, h, n)
    return [("ulp", cur, ulp), ("yaw", cur, yaw), ("move", cur, both)]


def pixels_of(w, h):
    if (w, h) in FRAMES_ALL:
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        return np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1)
    px = set()
    for x in range(w):
        px.update([(x, 0), (x, h - 1), (x, x * (h - 1) // (w - 1)), (x, (w - 1 - x) * (h - 1) // (w - 1))])
    for y in range(h):
        px.update([(0, y), (w - 1, y)])
    return np.array(sorted(px))


def reproject64(cur, prev, x, y, z):
    """Both maps in float64, from the views' own float32 fields."""
    def fields(v):
        f = tr.view_fields(v)
        m = f["m"].astype(np.float64)
        L = m[:9].reshape(3, 3).T
        n = f["n"]
        return L, np.linalg.inv(L), m[9:], float(f["xfov"]), float(f["yfov"]), float(f["clip_min"]), float(f["clip_max"]), \
            2.0 / f["width"], 2.0 / f["height"], 0.0 if n <= 1 else (n - 1) / (2.0 * n)
    L, _, T, xfov, yfov, cmin, cmax, pw, ph, cn = fields(cur)
    _, Li, Tp, xfov_p, yfov_p, cmin_p, cmax_p, pw_p, ph_p, cn_p = fields(prev)
    u, v = (x + cn) * pw - 1.0, (y + cn) * ph - 1.0
    yrot, xrot = xfov * 0.5 * -u, yfov * 0.5 * -v
    loc = np.stack([-np.cos(xrot) * np.sin(yrot), np.sin(xrot), -np.cos(xrot) * np.cos(yrot)], axis=-1)
    d = loc @ L.T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    far = z >= 1.0
    t = cmin + z * (cmax - cmin)
    p = np.where(far[:, None], d, T + t[:, None] * d - Tp)
    q = p @ Li.T
    e = q / np.linalg.norm(q, axis=-1, keepdims=True)
    xr, yr = np.arcsin(np.clip(e[:, 1], -1, 1)), np.arctan2(-e[:, 0], -e[:, 2])
    xf, yf = (-yr / (0.5 * xfov_p) + 1.0) / pw_p - cn_p, (-xr / (0.5 * yfov_p) + 1.0) / ph_p - cn_p
    zp = np.where(far, 1.0, (np.linalg.norm(p, axis=-1) - cmin_p) / (cmax_p - cmin_p))
    return xf, yf, zp


def host_reproject(bendy, cur, prev, px, z):
    out = (C.c_float * 3)()
    f, res = bendy.api.lib.bt_debug_reproject, np.zeros((len(px), 3), dtype=np.float32)
    cz = C.c_float(z)
    for i, (x, y) in enumerate(px):
        assert f(C.byref(cur), C.byref(prev), C.c_float(x), C.c_float(y), cz, out) == 0
        res[i] = out[0], out[1], out[2]
    return res


def worst_disagreement(bendy, frames):
    worst, worst_z = 0.0, 0.0
    for w, h in frames:
        px = pixels_of(w, h)
        for n in (0, 2):
            for name, cur, prev in pose_pairs(bendy, w, h, n):
                for z in DEPTHS:
                    got = host_reproject(bendy, cur, prev, px, z)
                    xf, yf, zp = reproject64(cur, prev, px[:, 0].astype(np.float64), px[:, 1].astype(np.float64),
                                             np.full(len(px), np.float64(np.float32(z))))
                    assert np.isfinite(got).all(), (w, h, n, name, z)
                    e = max(np.abs(got[:, 0] - xf).max(), np.abs(got[:, 1] - yf).max())
                    worst, worst_z = max(worst, e), max(worst_z, np.abs(got[:, 2] - zp).max())
                    # the numpy restatement of the same float32 lines agrees as closely
                    rx, ry, rz = tr.reproject(tr.prepare(cur), tr.prepare(prev), px[:, 0], px[:, 1], np.full(len(px), z, dtype=np.float32))
                    assert max(np.abs(rx - xf).max(), np.abs(ry - yf).max()) <= 4 * tr.EPS_PX, (w, h, n, name, z)
    return worst, worst_z


def test_reproject_matches_float64_small_frames(bendy):
    e, ez = worst_disagreement(bendy, FRAMES_ALL)
    print(f"largest disagreement, frames up to 64x36: {e:.3e} px, {ez:.3e} in z'")
    assert e <= 4 * tr.EPS_PX and ez <= 1e-6


def test_reproject_matches_float64_large_frames(bendy):
    e, ez = worst_disagreement(bendy, FRAMES_EDGE)
    print(f"largest disagreement, 768x512 and 3840x2160: {e:.3e} px, {ez:.3e} in z'")
    assert e <= 4 * tr.EPS_PX and ez <= 1e-6


@pytest.mark.parametrize("w,h", [(45, 35), (64, 36), (768, 512)])
@pytest.mark.parametrize("k", [1, 3, -2])
def test_yaw_by_k_pixels_shifts_columns(bendy, w, h, k):
    """The map is equi-angular in yaw: d_local = R_y(yrot) (0, sin xrot, -cos xrot) and yrot = -(xfov / 2) u, so a previous camera
    whose linear part is L R_y(theta), theta = k (xfov / 2) pw, sees the direction of pixel (x, y) at u + k pw: pixel (x, y) of the
    current view lies at (x + k, y) of the previous one, for every row and at any depth (the camera's position is the same)."""
    for n in (0, 2):
        cur = make_view(bendy, BASE_L, BASE_T, w, h, n)
        theta = k * (float(cur.xfov) / 2) * (2.0 / w)
        prev = make_view(bendy, BASE_L @ rot([0, 1, 0], theta), BASE_T, w, h, n)
        px = pixels_of(w, h) if (w, h) in FRAMES_ALL else pixels_of(w, h)[::7]
        for z in DEPTHS:
            got = host_reproject(bendy, cur, prev, px, z)
            assert np.abs(got[:, 0] - (px[:, 0] + k)).max() <= tr.EPS_PX and np.abs(got[:, 1] - px[:, 1]).max() <= tr.EPS_PX


def test_reproject_refuses_bad_views(bendy):
    good = make_view(bendy, BASE_L, BASE_T, 16, 16, 0)
    out = (C.c_float * 3)()
    for field, value in (("yfov", 0.0), ("xfov", -1.0), ("clip_max", 0.01), ("yfov", float("nan")), ("width", 0)):
        bad = good.copy()
        setattr(bad, field, value)
        assert bendy.api.lib.bt_debug_reproject(C.byref(good), C.byref(bad), 0.0, 0.0, 0.5, out) == -1
        assert bendy.api.lib.bt_debug_reproject(C.byref(bad), C.byref(good), 0.0, 0.0, 0.5, out) == -1
    flat = make_view(bendy, np.diag([1.0, 1.0, 0.0]), BASE_T, 16, 16, 0)
    assert bendy.api.lib.bt_debug_reproject(C.byref(good), C.byref(flat), 0.0, 0.0, 0.5, out) == -1
    assert bendy.reproject(good, good, 3.0, 5.0, 0.5)[:2] == pytest.approx((3.0, 5.0), abs=tr.EPS_PX)
