"""The compare stage (EXTENSION; include/bendy_hip.h, bt_compare) restated in numpy, operation by operation, in the
order csrc/bt_compare.hpp performs them: every float64 and float32 value here is the one the header's functions produce, so the
host entry point and the kernels are compared with `==` and `array_equal`.  Only psnr goes through a math library."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
FLT_MAX = np.finfo(f32).max
TILE = 16
C1, C2 = 1e-4, 9e-4
DEFAULTS = dict(epsilon=0.01, peak=1.0)
# the 11-tap window of sigma 1.5, as the literals of the header
_W = [float.fromhex(s) for s in ("0x1.0d956b52a1d70p-10", "0x1.f1fe01ae5a5b8p-8", "0x1.26eb175d83f67p-5", "0x1.bff0fe8e98418p-4",
                                 "0x1.b43c3f52b19f2p-3", "0x1.106560aa892c0p-2")]
W = _W + _W[4::-1]
FIELDS = ("pixels", "valid", "nonfinite", "max_index", "mse", "rel_mse", "ssim", "max_abs", "psnr")


def mean(X, n):
    """What Buffer.mean() computes: rgb * (1 / n) in float32."""
    with np.errstate(all="ignore"):
        return np.asarray(X, dtype=f32)[..., :3] * (f32(1.0) / f32(n))


def point(X, nx, Y, ny, epsilon):
    """Steps 1 and 2 -> (se, re, m, bad, E, v), v of shape [h, w, 2]."""
    x, y = mean(X, nx), mean(Y, ny)
    with np.errstate(all="ignore"):
        bad = ~((np.abs(x) < np.inf).all(-1) & (np.abs(y) < np.inf).all(-1))
        xd, yd = x.astype(f64), y.astype(f64)
        d = xd - yd
        e = d * d
        q = e / (yd * yd + f64(epsilon))
        se = np.where(bad, 0.0, (e[..., 0] + e[..., 1]) + e[..., 2])
        re = np.where(bad, 0.0, (q[..., 0] + q[..., 1]) + q[..., 2])
        m = np.where(bad, 0.0, np.abs(d).max(-1))
        E = np.where(re < f64(FLT_MAX), re.astype(f32), FLT_MAX).astype(f32)
        E[bad] = f32(-0.0)                     # == 0; the sign bit keeps the pixel out of the tail and paints it magenta
        v = np.zeros(x.shape[:2] + (2,), dtype=f64)
        for side, c in enumerate((x, y)):
            Yf = (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]
            Yc = np.where(Yf > 0, np.where(Yf < FLT_MAX, Yf, FLT_MAX), f32(0.0)).astype(f32)
            Yc[bad] = 0.0
            Yd = Yc.astype(f64)
            v[..., side] = Yd / (1.0 + Yd)
    return se, re, m, bad, E, v


def blur(P, axis):
    """acc = 0; acc = acc + W[k] * a[clamp(i + k - 5)], k = 0 .. 10, along `axis` of a stack of planes [5, h, w]."""
    n = P.shape[axis]
    pad = [(0, 0)] * P.ndim
    pad[axis] = (5, 5)
    Q = np.pad(P, pad, mode="edge")
    acc = np.zeros_like(P)
    for k in range(11):
        acc = acc + W[k] * np.take(Q, range(k, k + n), axis=axis)
    return acc


def ssim_plane(v):
    vx, vy = v[..., 0], v[..., 1]
    P = np.stack([vx, vy, vx * vx, vy * vy, vx * vy])
    mx, my, xx, yy, xy = blur(blur(P, 2), 1)
    sx = xx - mx * mx
    sy = yy - my * my
    cxy = xy - mx * my
    return ((2.0 * (mx * my) + C1) * (2.0 * cxy + C2)) / (((mx * mx + my * my) + C1) * ((sx + sy) + C2))


def tile_partials(a):
    """Step 4's tree per 16 x 16 tile, 0.0 outside the frame -> the partials in tile order."""
    h, w = a.shape
    ty, tx = -(-h // TILE), -(-w // TILE)
    p = np.zeros((ty * TILE, tx * TILE), dtype=f64)
    p[:h, :w] = a
    t = p.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty * tx, TILE * TILE).copy()
    stride = 128
    while stride >= 1:
        t[:, :stride] = t[:, :stride] + t[:, stride:2 * stride]
        stride //= 2
    return t[:, 0].copy()


def frame_sum(a):
    return f64(np.cumsum(tile_partials(a))[-1])      # cumsum adds one after another


def measure(X, Y, nx=1, ny=1, epsilon=0.01, peak=1.0):
    """-> dict of the bt_compare_stats fields plus the planes E, v, s."""
    se, re, m, bad, E, v = point(X, nx, Y, ny, epsilon)
    s = ssim_plane(v)
    pixels = int(bad.size)
    nonfinite = int(bad.sum())
    valid = pixels - nonfinite
    mse = float(frame_sum(se) / f64(3 * valid)) if valid else 0.0
    rel = float(frame_sum(re) / f64(3 * valid)) if valid else 0.0
    return dict(pixels=pixels, valid=valid, nonfinite=nonfinite, max_index=int(np.argmax(m.ravel())), mse=mse, rel_mse=rel,
                ssim=float(frame_sum(s) / f64(pixels)), max_abs=float(m.max()),
                psnr=math.inf if mse == 0.0 else 10.0 * math.log10(peak * peak / mse), E=E, v=v, s=s)


def tail_rank(fraction, valid):
    want = fraction * float(valid)
    k = int(want)
    if k < want:
        k += 1
    return min(max(k, 1), valid)


def tail(E, fraction, details=False):
    """Step 6 -> (share, threshold)."""
    ok = ~np.signbit(E)
    vals = E[ok]
    valid = int(vals.size)
    if valid == 0:
        return (0.0, 0.0, dict(k=0, c_gt=0)) if details else (0.0, 0.0)
    k = tail_rank(fraction, valid)
    T = np.sort(vals)[valid - k]
    gt = ok & (E > T)
    S_gt = frame_sum(np.where(gt, E.astype(f64), 0.0))
    S_all = frame_sum(np.where(ok, E.astype(f64), 0.0))
    c_gt = int(gt.sum())
    share = float((S_gt + f64(k - c_gt) * f64(T)) / S_all) if S_all != 0.0 else 0.0
    return (share, float(T), dict(k=k, c_gt=c_gt, S_all=float(S_all))) if details else (share, float(T))


def error_map(E, scale=1.0):
    """Step 7 -> uint8 [h, w, 4]."""
    bad = np.signbit(E)
    with np.errstate(all="ignore"):
        q = np.abs(E) / f32(scale)
    t = np.where(q < 1, q, f32(1.0)).astype(f32)
    t3 = f32(3.0) * t
    clamp01 = lambda a: np.where(a > 0, np.where(a < 1, a, f32(1.0)), f32(0.0)).astype(f32)
    r, g, b = np.where(t3 < 1, t3, f32(1.0)).astype(f32), clamp01(t3 - f32(1.0)), clamp01(t3 - f32(2.0))
    out = np.empty(E.shape + (4,), dtype=np.uint8)
    for c, ch in enumerate((r, g, b)):
        out[..., c] = (ch * f32(255.0) + f32(0.5)).astype(np.uint8)
    out[..., 3] = 255
    out[bad] = (255, 0, 255, 255)
    return out


def rel_mse_numpy(x, y):
    """The float64 formula of the existing tests and tools, on means."""
    x, y = x[..., :3].astype(f64), y[..., :3].astype(f64)
    return float(np.mean((x - y) ** 2 / (y ** 2 + 0.01)))


# ---- inputs ----
def spots(w, h):
    """The first pixel, the last one and pixel 256 (where the frame has one)."""
    n = w * h
    return sorted({0, n - 1} | ({256} if n > 256 else set()))


def make_pair(w, h, seed, noise=0.05, nx=1, ny=1, poison=None):
    """-> (X, Y) running sums [h, w, 4]: log-normal colour over 2^-20 .. 2^20, X = Y with noise of relative size `noise`.
    poison = "nonfinite": NaN, +inf and -inf at the spots; "big": 3e38 there."""
    rng = np.random.default_rng(seed)
    y = np.exp2(rng.uniform(-20.0, 20.0, size=(h, w, 3)))
    x = y * (1.0 + noise * rng.standard_normal((h, w, 3))) if noise else y.copy()
    X, Y = np.empty((h, w, 4), dtype=f32), np.empty((h, w, 4), dtype=f32)
    X[..., :3], Y[..., :3] = (x * nx).astype(f32), (y * ny).astype(f32)
    X[..., 3], Y[..., 3] = rng.uniform(size=(h, w)).astype(f32), 1.0
    fx, fy = X.reshape(-1, 4), Y.reshape(-1, 4)
    for n, p in enumerate(spots(w, h)):
        if poison == "nonfinite":
            (fx if n % 2 == 0 else fy)[p, n % 3] = (np.nan, np.inf, -np.inf)[n % 3]
        elif poison == "big":
            (fx if n % 2 == 0 else fy)[p, n % 3] = 3e38
    return X, Y
