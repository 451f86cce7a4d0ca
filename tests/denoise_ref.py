"""Float32 numpy restatement of the AOV-guided a-trous denoiser (bendy_tracer_amd/csrc/bt_denoise.hip).

Test infrastructure: every product and sum is formed in the kernel's order (taps dy outer, dx inner; the weight
((((h[dx] h[dy]) w_n) w_z) w_c); |d|^2 = (r^2 + g^2) + b^2), vectorised over pixels only, so that GPU and reference
differ by the ulps of expf / powf alone."""
import numpy as np

f32 = np.float32
H5 = [f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16)]
DEFAULTS = dict(levels=2, sigma_color=16.0, sigma_normal=16.0, sigma_depth=1.0, eps_albedo=1e-3)


def _albedo_factor(albedo, n_a, eps):
    a = albedo[..., :3] / f32(n_a)
    return np.where(a > f32(eps), a, f32(1.0)).astype(f32)


def prepare(color, n_c, albedo=None, n_a=1, normal=None, n_n=1, depth=None, n_d=1, eps_albedo=1e-3):
    """-> e [H, W, 3], guide normal [H, W, 3] (0 = miss / no guide), guide depth [H, W]."""
    color = np.asarray(color, f32)
    h, w, _ = color.shape
    e = color[..., :3] / f32(n_c)
    if albedo is not None:
        e = e / _albedo_factor(np.asarray(albedo, f32), n_a, eps_albedo)
    nrm = np.zeros((h, w, 3), f32)
    if normal is not None:
        v = np.asarray(normal, f32)[..., :3] / f32(n_n)
        l2 = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]
        ok = l2 > f32(1e-12)
        l = np.sqrt(np.where(ok, l2, f32(1.0)))
        nrm = np.where(ok[..., None], v / l[..., None], f32(0.0)).astype(f32)
    z = np.zeros((h, w), f32)
    if depth is not None:
        z = np.asarray(depth, f32)[..., 0] / f32(n_d)
    return e.astype(f32), nrm, z.astype(f32)


def atrous_pass(e, nrm, z, level, sigma_color, sigma_normal, sigma_depth):
    """One level (step 2^level) of the filter; taps outside the frame are skipped."""
    h, w, _ = e.shape
    s = 1 << level
    inv_color = f32(4 ** level) / (f32(sigma_color) * f32(sigma_color))
    sn, sd = f32(sigma_normal), f32(sigma_depth)
    p_zero = (nrm[..., 0] == 0) & (nrm[..., 1] == 0) & (nrm[..., 2] == 0)
    zs = sd * z * f32(s)
    acc = np.zeros((h, w, 3), f32)
    wsum = np.zeros((h, w), f32)
    ys, xs = np.arange(h), np.arange(w)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for dy in range(-2, 3):
            qy = ys + dy * s
            vy = (qy >= 0) & (qy < h)
            qyc = np.clip(qy, 0, h - 1)
            for dx in range(-2, 3):
                qx = xs + dx * s
                vx = (qx >= 0) & (qx < w)
                qxc = np.clip(qx, 0, w - 1)
                inside = vy[:, None] & vx[None, :]
                eq = e[qyc][:, qxc]
                nq = nrm[qyc][:, qxc]
                zq = z[qyc][:, qxc]
                q_zero = (nq[..., 0] == 0) & (nq[..., 1] == 0) & (nq[..., 2] == 0)
                d = nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1] + nrm[..., 2] * nq[..., 2]
                wn = np.power(np.maximum(f32(0.0), d), sn)
                wn = np.where(~p_zero & ~q_zero, wn, np.where(p_zero & q_zero, f32(1.0), f32(0.0))).astype(f32)
                m = f32(max(abs(dx), abs(dy)))
                wz = np.exp(-np.abs(z - zq) / (zs * m + f32(1e-6)))
                dr, dg, db = e[..., 0] - eq[..., 0], e[..., 1] - eq[..., 1], e[..., 2] - eq[..., 2]
                wc = np.exp(-(dr * dr + dg * dg + db * db) * inv_color)
                wt = H5[dx + 2] * H5[dy + 2] * wn * wz * wc
                wt = np.where(inside, wt, f32(0.0)).astype(f32)
                # a skipped tap adds exactly 0 (+0.0 keeps every partial sum bit-identical to not adding)
                acc = acc + np.where(inside[..., None], wt[..., None] * eq, f32(0.0))
                wsum = wsum + wt
    return (acc / wsum[..., None]).astype(f32)


def denoise(color, n_c, albedo=None, n_a=1, normal=None, n_n=1, depth=None, n_d=1, **params):
    """The whole filter: [H, W, 4] running sums -> [H, W, 4] mean (alpha = the colour buffer's alpha)."""
    p = {**DEFAULTS, **params}
    color = np.asarray(color, f32)
    out = np.empty_like(color)
    out[..., 3] = color[..., 3]
    if p["levels"] == 0:
        out[..., :3] = color[..., :3] / f32(n_c)
        return out
    e, nrm, z = prepare(color, n_c, albedo, n_a, normal, n_n, depth, n_d, p["eps_albedo"])
    for i in range(p["levels"]):
        e = atrous_pass(e, nrm, z, i, p["sigma_color"], p["sigma_normal"], p["sigma_depth"])
    if albedo is not None:
        e = e * _albedo_factor(np.asarray(albedo, f32), n_a, p["eps_albedo"])
    out[..., :3] = e
    return out
