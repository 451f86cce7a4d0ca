"""float32 numpy restatement of temporal accumulation with reprojection (EXTENSION; include/bendy_hip.h bt_temporal):
the two maps of csrc/bt_view.hpp and the per-pixel definition of csrc/bt_temporal.hip, operation by operation in the kernel's
order.  The two differ by the ulps of sin / cos / asin / atan2 only, which is what EPS_PX bounds.  Besides the frame and the
new history `accumulate` returns a per-pixel `fragile` mask: pixels where a decision (a tap's depth or normal test, W against
1e-3, a tap being inside the frame) lies so close to flipping that those ulps may decide it."""
import numpy as np

f32 = np.float32

# Largest disagreement, in pixels, between bt_view.hpp's float32 maps and their float64 restatement over the pixel sets, pose
# pairs, sub-sampling modes and depths of tests/test_view_projection.py (frames up to 3840x2160), as measured there: 1.09e-3 px, reached at 3840x2160 (1.3e-5 px on frames up to 64x36).
EPS_PX = 1.1e-3

DEFAULTS = dict(alpha_min=0.05, max_history=256.0, depth_tolerance=0.05, normal_min=0.5)      # bt_temporal_params_default


def view_fields(v):
    """A View (ctypes) as plain numpy / python values."""
    return dict(m=np.array(list(v.to_world), dtype=f32), yfov=f32(v.yfov), xfov=f32(v.xfov), clip_min=f32(v.clip_min),
                clip_max=f32(v.clip_max), width=int(v.width), height=int(v.height), n=int(v.subsample_n))


def prepare(v):
    """btview::prepare: L^-1 by the adjugate in float64, rounded to float32; pw, ph and the footprint's centre offset."""
    p = view_fields(v)
    m = p["m"].astype(np.float64)
    a, b, c, d, e, f, g, h, i = m[0], m[3], m[6], m[1], m[4], m[7], m[2], m[5], m[8]
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    assert abs(det) >= 1e-12
    inv = np.zeros(9)
    inv[0], inv[3], inv[6] = (e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det
    inv[1], inv[4], inv[7] = (f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det
    inv[2], inv[5], inv[8] = (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det
    p["inv"] = inv.astype(f32)
    p["pw"] = f32(2.0) * (f32(1.0) / f32(p["width"]))
    p["ph"] = f32(2.0) * (f32(1.0) / f32(p["height"]))
    n = p["n"]
    p["cn"] = f32(0.0) if n <= 1 else f32(n - 1) / f32(2 * n)
    return p


def _mul3(m, p):
    return [(m[0] * p[0] + m[3] * p[1]) + m[6] * p[2], (m[1] * p[0] + m[4] * p[1]) + m[7] * p[2],
            (m[2] * p[0] + m[5] * p[1]) + m[8] * p[2]]


def forward(V, x, y):
    x, y = np.asarray(x, dtype=f32), np.asarray(y, dtype=f32)
    u, v = (x + V["cn"]) * V["pw"] - f32(1.0), (y + V["cn"]) * V["ph"] - f32(1.0)
    yrot, xrot = V["xfov"] * f32(0.5) * -u, V["yfov"] * f32(0.5) * -v
    cx = np.cos(xrot)
    w = _mul3(V["m"], [-cx * np.sin(yrot), np.sin(xrot), -cx * np.cos(yrot)])
    l = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    return [w[0] / l, w[1] / l, w[2] / l]


def inverse(V, p):
    with np.errstate(all="ignore"):
        q = _mul3(V["inv"], p)
        l = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
        ex, ey, ez = q[0] / l, q[1] / l, q[2] / l
        xrot, yrot = np.arcsin(np.minimum(np.maximum(ey, f32(-1.0)), f32(1.0))), np.arctan2(-ex, -ez)
        u, v = -yrot / (f32(0.5) * V["xfov"]), -xrot / (f32(0.5) * V["yfov"])
        return (u + f32(1.0)) / V["pw"] - V["cn"], (v + f32(1.0)) / V["ph"] - V["cn"]


def reproject(cur, prev, x, y, z):
    """btview::reproject on arrays: (x_f, y_f, z'), all float32."""
    z = np.asarray(z, dtype=f32)
    d = forward(cur, x, y)
    far = z >= f32(1.0)
    t = cur["clip_min"] + z * (cur["clip_max"] - cur["clip_min"])
    T, Tp = cur["m"][9:], prev["m"][9:]
    p = [(T[k] + t * d[k]) - Tp[k] for k in range(3)]
    r = np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
    xa, ya = inverse(prev, p)
    xb, yb = inverse(prev, d)
    zp = (r - prev["clip_min"]) / (prev["clip_max"] - prev["clip_min"])
    return np.where(far, xb, xa).astype(f32), np.where(far, yb, ya).astype(f32), np.where(far, f32(1.0), zp).astype(f32)


def same_view(a, b):
    return bytes(a) == bytes(b)


def _close(a, b, rel=1e-3):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.maximum(np.abs(a), np.abs(b))
    return (m > 0) & (np.abs(a - b) <= rel * m)


def accumulate(state, view, color, nc, normal, nn, depth, nd, eps_px=EPS_PX, **params):
    """One bt_temporal_accumulate_device call.  `state`: None (no history) or what an earlier call returned as its second
    value; color / normal / depth: float32 [H, W, 4] running sums (normal may be None).  Returns (out [H, W, 4], state,
    info) with info = dict(fragile, reset: bool [H, W]; xf, yf, zp)."""
    P = {**DEFAULTS, **params}
    H, W = color.shape[:2]
    nc_, nd_ = f32(nc), f32(nd)
    with np.errstate(all="ignore"):
        c = color[..., :3] / nc_
        g = np.zeros((H, W, 4), dtype=f32)
        if normal is not None:
            v = normal[..., :3] / f32(nn)
            l2 = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]
            ok = l2 > f32(1e-12)
            l = np.sqrt(np.where(ok, l2, f32(1.0)))
            g[..., :3] = np.where(ok[..., None], v / l[..., None], f32(0.0))
        g[..., 3] = depth[..., 0] / nd_
        z = g[..., 3]
        far = z >= f32(1.0)
        reset_rgb, reset_len = c, np.full((H, W), nc_, dtype=f32)
        fragile = np.zeros((H, W), dtype=bool)
        ys, xs = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
        xf, yf, zp = xs, ys, z
        if state is None:
            rgb, length, reset = reset_rgb, reset_len, np.ones((H, W), dtype=bool)
        else:
            static = same_view(state["view"], view)
            if not static:
                xf, yf, zp = reproject(prepare(view), prepare(state["view"]), xs, ys, z)
            hist, guide = state["hist"], state["guide"]
            a_min, h_max = f32(P["alpha_min"]), f32(P["max_history"])
            ztol = f32(P["depth_tolerance"]) * zp
            np_zero = (g[..., 0] == 0) & (g[..., 1] == 0) & (g[..., 2] == 0)

            def in_range(px, py):
                return (px > f32(-1.0)) & (px < f32(W)) & (py > f32(-1.0)) & (py < f32(H))

            def tap_pattern(px, py):
                """which of the four taps are inside the frame, as a 4-bit number per pixel (0 if out of range)"""
                rng = in_range(px, py)
                x0 = np.floor(np.where(rng, px, f32(0.0))).astype(np.int64)
                y0 = np.floor(np.where(rng, py, f32(0.0))).astype(np.int64)
                bits = np.zeros(px.shape, dtype=np.int64)
                for j in range(2):
                    for i in range(2):
                        inside = (x0 + i >= 0) & (x0 + i < W) & (y0 + j >= 0) & (y0 + j < H)
                        bits |= inside.astype(np.int64) << (2 * j + i)
                return np.where(rng, bits, 0)

            rng = in_range(xf, yf)
            x0f, y0f = np.floor(np.where(rng, xf, f32(0.0))), np.floor(np.where(rng, yf, f32(0.0)))
            fx, fy = np.where(rng, xf, f32(0.0)) - x0f, np.where(rng, yf, f32(0.0)) - y0f
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            s = [np.zeros((H, W), dtype=f32) for _ in range(5)]           # r, g, b, length, weight
            for j in range(2):
                for i in range(2):
                    qx, qy = x0 + i, y0 + j
                    w = (fx if i else f32(1.0) - fx) * (fy if j else f32(1.0) - fy)
                    inside = rng & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & (w != 0)
                    cx_, cy_ = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    gq, hq = guide[cy_, cx_], hist[cy_, cx_]
                    dz = np.abs(zp - gq[..., 3])
                    pass_z = np.where(far, gq[..., 3] >= f32(1.0), (gq[..., 3] < f32(1.0)) & (dz <= ztol))
                    fragile |= inside & ~far & (gq[..., 3] < f32(1.0)) & _close(dz, ztol)
                    pass_n = np.ones((H, W), dtype=bool)
                    if normal is not None:
                        nq_zero = (gq[..., 0] == 0) & (gq[..., 1] == 0) & (gq[..., 2] == 0)
                        dot = (g[..., 0] * gq[..., 0] + g[..., 1] * gq[..., 1]) + g[..., 2] * gq[..., 2]
                        pass_n = np.where(np_zero | nq_zero, np_zero & nq_zero, dot >= f32(P["normal_min"]))
                        fragile |= inside & ~np_zero & ~nq_zero & _close(dot, f32(P["normal_min"]))
                    keep = inside & pass_z & pass_n
                    if static:                                        # the pixel's own history, untested: (x, y) has fx = fy = 0
                        keep, fragile[...] = inside, False
                    for k in range(4):
                        s[k] = np.where(keep, s[k] + w * hq[..., k], s[k])
                    s[4] = np.where(keep, s[4] + w, s[4])
            sw = s[4]
            if not static:
                fragile |= _close(sw, f32(1e-3))
            blend = sw >= f32(1e-3)
            swd = np.where(blend, sw, f32(1.0))
            m = np.stack([s[0] / swd, s[1] / swd, s[2] / swd], axis=-1)
            h = s[3] / swd
            N = np.minimum(h + nc_, h_max)
            a = np.minimum(f32(1.0), np.maximum(nc_ / N, a_min))
            rgb = np.where(blend[..., None], m + (c - m) * a[..., None], reset_rgb)
            length = np.where(blend, N, reset_len)
            reset = ~blend
            if not static:
                d = f32(4.0 * eps_px)
                base = tap_pattern(xf, yf)
                for sx in (-d, d):
                    for sy in (-d, d):
                        fragile |= tap_pattern(xf + sx, yf + sy) != base
                fragile |= ~np.isfinite(xf) | ~np.isfinite(yf)
    out = np.concatenate([rgb, color[..., 3:4]], axis=-1).astype(f32)
    new_state = dict(hist=np.concatenate([rgb, length[..., None]], axis=-1).astype(f32), guide=g, view=view)
    return out, new_state, dict(fragile=fragile, reset=reset, xf=xf, yf=yf, zp=zp)
