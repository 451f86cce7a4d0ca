"""The upscale stage (EXTENSION; include/bendy_hip.h, bt_upscale) restated in numpy, operation by operation as
csrc/bt_upscale.hpp states it: float32 pixels in the order written, float64 tables.  The host entry point and the GPU are held
to this bit for bit (tests/test_upscale_host.py, tests/test_gpu_upscale.py); tests/test_upscale_ref.py holds this file to its
properties.  A guide is None, an array of sums with count 1 or (array, count)."""
import math

import numpy as np

from glare_ref import make_frame, sanitise, ulps  # noqa: F401  (step 1's colour is the glare stage's; the frames and ulps are shared)

f32 = np.float32
# bt_upscale_params_default
DEFAULTS = dict(sigma_depth=0.1, sigma_albedo=0.1, normal_squarings=3, min_weight=0.01, max_value=65536.0)


# ---- step 1 ----
def fin(v):
    """|v| < inf ? v : 0 (a NaN fails the compare)."""
    v = np.asarray(v, dtype=f32)
    with np.errstate(all="ignore"):
        return np.where(np.abs(v) < f32(np.inf), v, f32(0.0)).astype(f32)


def _pair(g):
    if g is None:
        return None, 1
    arr, n = g if isinstance(g, tuple) else (g, 1)
    return np.asarray(arr, dtype=f32), int(n)


def prepare(shape, albedo, normal, depth):
    """-> (n [.., 3], a [.., 3], z [..]) of one frame's guides; an absent guide is zeros."""
    with np.errstate(all="ignore"):
        A, na = _pair(albedo)
        a = np.zeros(shape + (3,), dtype=f32) if A is None else fin(A[..., :3] * (f32(1.0) / f32(na)))
        N, nn = _pair(normal)
        if N is None:
            n = np.zeros(shape + (3,), dtype=f32)
        else:
            v = fin(N[..., :3] * (f32(1.0) / f32(nn)))
            l = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
            ok = l > f32(1e-12)
            s = np.sqrt(np.where(ok, l, f32(1.0)).astype(f32))
            n = np.where(ok[..., None], v / s[..., None], f32(0.0)).astype(f32)
        Z, nz = _pair(depth)
        z = np.zeros(shape, dtype=f32) if Z is None else fin(Z[..., 0] * (f32(1.0) / f32(nz)))
    return n, a, z


def planes(color, samples, lo, max_value=65536.0):
    """The three prepared lo planes as the handle keeps them: (c.rgb, z), (n.xyz, 0), (a.rgb, 0), each [h, w, 4]."""
    c = sanitise(color, samples, max_value)
    n, a, z = prepare(c.shape[:2], *lo)
    zero = np.zeros(c.shape[:2] + (1,), dtype=f32)
    return (np.concatenate([c[..., :3], z[..., None]], axis=-1), np.concatenate([n, zero], axis=-1), np.concatenate([a, zero], axis=-1))


# ---- step 2 ----
def axis_table(src, dst):
    """-> (first int64 [dst] = x0 - 1 unclamped, weights float32 [dst, 8] = u1_0 .. u1_3, u2_0 .. u2_3, nearest int64 [dst])."""
    ratio = float(src) / float(dst)
    first, near = np.zeros(dst, dtype=np.int64), np.zeros(dst, dtype=np.int64)
    w = np.zeros((dst, 8), dtype=f32)
    for i in range(dst):
        c = (i + 0.5) * ratio - 0.5
        x0 = math.floor(c)
        f = c - x0
        first[i] = x0 - 1
        for t in range(4):
            d = abs((t - 1) - f)
            w[i, t] = f32(max(0.0, 1.0 - d))
            w[i, 4 + t] = f32(max(0.0, 1.0 - d * 0.5))
        near[i] = min(src - 1, math.floor((i + 0.5) * ratio))
    return first, w, near


# ---- steps 3 to 5 ----
def upscale(color, samples, width, height, lo=None, hi=None, sigma_depth=0.1, sigma_albedo=0.1, normal_squarings=3, min_weight=0.01,
            max_value=65536.0, tables=None, details=False):
    """-> the upscaled mean [height, width, 4] (alpha = the input's at the nearest texel); with details=True also a dict: `tier`
    (int [height, width], 1 .. 3) and `counts` = (tier 2, tier 3, pixels).  `tables`: (x table, y table) as axis_table returns
    them -- the library's own, or None for this module's."""
    C = np.asarray(color, dtype=f32)
    h, w = C.shape[:2]
    W, H = int(width), int(height)
    assert W >= w and H >= h, "the stage does not reduce"
    lo, hi = lo or (None, None, None), hi or (None, None, None)
    assert all((a is None) == (b is None) for a, b in zip(lo, hi)), "a guide pair needs both sizes"
    pcz, pn, pa = planes(C, samples, lo, max_value)
    n_p, a_p, z_p = prepare((H, W), *hi)
    (fx, wx, nx), (fy, wy, ny) = tables if tables is not None else (axis_table(w, W), axis_table(h, H))
    sd, mw = f32(sigma_depth), f32(min_weight)
    k_a = f32(1.0) / (f32(sigma_albedo) * f32(sigma_albedo))
    one, zero = f32(1.0), f32(0.0)
    with np.errstate(all="ignore"):
        z_den = sd * z_p + f32(1e-6)
        miss_p = (n_p == 0).all(axis=-1)
        A1, A2, A0 = (np.zeros((H, W, 3), dtype=f32) for _ in range(3))
        D1, D2, D0 = (np.zeros((H, W), dtype=f32) for _ in range(3))
        for ty in range(4):
            qy = np.clip(np.asarray(fy, dtype=np.int64) + ty, 0, h - 1)[:, None]
            for tx in range(4):
                qx = np.clip(np.asarray(fx, dtype=np.int64) + tx, 0, w - 1)[None, :]
                cz, n_q, a_q = pcz[qy, qx], pn[qy, qx][..., :3], pa[qy, qx][..., :3]
                miss_q = (n_q == 0).all(axis=-1)
                m = (n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2]
                m = np.where(m > 0, m, zero).astype(f32)
                for _ in range(int(normal_squarings)):
                    m = m * m
                g_n = np.where(miss_p & miss_q, one, np.where(miss_p | miss_q, zero, m)).astype(f32)
                t = np.abs(z_p - cz[..., 3]) / z_den
                g_z = one / (one + t * t)
                d = a_p - a_q
                s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                g_a = one / (one + s * k_a)
                g = (g_n * g_z) * g_a
                s1 = wy[:, ty][:, None] * wx[:, tx][None, :]
                s2 = wy[:, 4 + ty][:, None] * wx[:, 4 + tx][None, :]
                w1, w2 = s1 * g, s2 * g
                c_q = cz[..., :3]
                A1, D1 = A1 + w1[..., None] * c_q, D1 + w1
                A2, D2 = A2 + w2[..., None] * c_q, D2 + w2
                A0, D0 = A0 + s1[..., None] * c_q, D0 + s1
        t1 = D1 > mw
        t2 = ~t1 & (D2 > mw)
        tier = np.where(t1, 1, np.where(t2, 2, 3))
        num = np.where(t1[..., None], A1, np.where(t2[..., None], A2, A0))
        den = np.where(t1, D1, np.where(t2, D2, D0))
        rgb = (num / den[..., None]).astype(f32)
    out = np.concatenate([rgb, C[np.asarray(ny)[:, None], np.asarray(nx)[None, :], 3][..., None]], axis=-1).astype(f32)
    if details:
        return out, dict(tier=tier, counts=(int((tier == 2).sum()), int((tier == 3).sum()), W * H))
    return out


# ---- frames for the tests ----
def make_guides(width, height, seed=1, poison=True, samples=(1, 1, 1)):
    """Random (albedo, normal, depth) sums of the given counts: albedo in [0, 1), unit normals with about one in eight zero (a
    miss), depth in [0.5, 20); with `poison` NaN, -3, -inf, +inf and 3e38 visit the first pixel, the last one and pixel 256."""
    rng = np.random.default_rng(seed)
    albedo = np.ones((height, width, 4), dtype=f32)
    albedo[..., :3] = rng.uniform(0.0, 1.0, size=(height, width, 3))
    normal = np.ones((height, width, 4), dtype=f32)
    v = rng.normal(size=(height, width, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    v[rng.uniform(size=(height, width)) < 0.125] = 0.0
    normal[..., :3] = v
    depth = np.ones((height, width, 4), dtype=f32)
    depth[..., :3] = rng.uniform(0.5, 20.0, size=(height, width, 1))
    out = []
    bad = [f32(np.nan), f32(-3.0), f32(-np.inf), f32(np.inf), f32(3e38)]
    for k, (g, n) in enumerate(zip((albedo, normal, depth), samples)):
        g[..., :3] *= f32(n)
        if poison:
            flat = g.reshape(-1, 4)
            for j, at in enumerate(p for p in (0, flat.shape[0] - 1, 256) if p < flat.shape[0]):
                for ch in range(3):
                    flat[at, ch] = bad[(j + ch + k) % 5]
        out.append((g, n))
    return tuple(out)


def subset(guides, mask):
    """The pairs of `guides` whose bit is set in `mask` (1 albedo, 2 normal, 4 depth), the others None."""
    return tuple(g if mask >> k & 1 else None for k, g in enumerate(guides))


def coherent_pair(w, h, W, H, seed=1, poison=True, samples=(1, 1, 1)):
    """Guides of a lo and a hi frame that have something to do with each other: piecewise-constant regions laid out in the unit
    square, sampled at both sizes, so that taps match their output pixel here and miss it there.  -> (lo, hi)."""
    rng = np.random.default_rng(seed)
    K = 5
    alb = rng.uniform(0.0, 1.0, size=(K, 3)).astype(f32)
    nor = rng.normal(size=(K, 3))
    nor /= np.linalg.norm(nor, axis=-1, keepdims=True)
    nor[0] = 0.0                                                   # region 0 is a miss
    dep = rng.uniform(0.5, 20.0, size=K).astype(f32)
    cx, cy = rng.uniform(size=K), rng.uniform(size=K)

    def at(ww, hh, salt):
        x, y = (np.arange(ww) + 0.5) / ww, (np.arange(hh) + 0.5) / hh
        lab = np.argmin((x[None, :, None] - cx) ** 2 + (y[:, None, None] - cy) ** 2, axis=-1)
        r = np.random.default_rng(seed * 7 + salt)
        frames = []
        for k, (vals, n) in enumerate(zip((alb, nor.astype(f32), dep[:, None].repeat(3, 1)), samples)):
            g = np.ones((hh, ww, 4), dtype=f32)
            g[..., :3] = vals[lab] * f32(n)
            if k == 2:
                g[..., :3] *= (1.0 + 0.01 * r.uniform(-1, 1, size=(hh, ww, 1))).astype(f32)
            frames.append(g)
        if poison:
            bad = [f32(np.nan), f32(-3.0), f32(-np.inf), f32(np.inf), f32(3e38)]
            for k, g in enumerate(frames):
                flat = g.reshape(-1, 4)
                for j, p in enumerate(q for q in (0, flat.shape[0] - 1, 256) if q < flat.shape[0]):
                    for ch in range(3):
                        flat[p, ch] = bad[(j + ch + k + salt) % 5]
        return tuple((g, n) for g, n in zip(frames, samples))

    return at(w, h, 0), at(W, H, 1)
