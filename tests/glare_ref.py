"""numpy restatement of the glare stage (EXTENSION; include/bendy_hip.h bt_glare): sanitise, the down pyramid, the
level weights, up-and-accumulate and the composite, operation by operation in the order csrc/bt_glare.hpp has them.  Every
float32 step is one correctly rounded numpy float32 operation on whole planes; the weights are float64 products and one
float64 division each, rounded once to float32.  Planes are [h, w, 4] with a fourth channel of 0, as the device's."""
import numpy as np

f32 = np.float32

MAX_LEVELS = 16
# bt_glare_params_default
DEFAULTS = dict(levels=6, spread=1.0, strength=0.08, max_value=65536.0)


def effective_levels(levels, width, height):
    """L = min(levels, bit_length(max(width, height) - 1)): the halvings until both sides are 1."""
    return min(int(levels), (max(int(width), int(height)) - 1).bit_length())


def half_side(side):
    return (side + 1) // 2


def sanitise(rgba, samples, max_value):
    """r = 1 / n; c = rgb * r; s = c >= 0 ? c : 0; s = s < max_value ? s : max_value; the fourth channel is 0."""
    a = np.asarray(rgba, dtype=f32)
    r = f32(1.0) / f32(samples)
    with np.errstate(all="ignore"):
        c = a[..., :3] * r
        s = np.where(c >= 0, c, f32(0.0)).astype(f32)
        s = np.where(s < f32(max_value), s, f32(max_value)).astype(f32)
    return np.concatenate([s, np.zeros(a.shape[:-1] + (1,), dtype=f32)], axis=-1)


def _down_axis(p, axis):
    side = p.shape[axis]
    i = np.arange(half_side(side), dtype=np.int64)
    a, b, c, d = (np.take(p, np.clip(2 * i - 1 + t, 0, side - 1), axis=axis) for t in range(4))
    t = b + c
    return (((a + d) + t) + (t + t)) * f32(0.125)


def down(p):
    """[1 3 3 1] / 8 along x, then along y, each decimating by two."""
    return _down_axis(_down_axis(p, 1), 0)


def _up_axis(c, fine, axis):
    cs = c.shape[axis]
    x = np.arange(fine, dtype=np.int64)
    near = x >> 1
    far = np.clip(np.where(x & 1, near + 1, near - 1), 0, cs - 1)
    n, f = np.take(c, near, axis=axis), np.take(c, far, axis=axis)
    return ((f + n) + (n + n)) * f32(0.25)


def up(c, height, width):
    """[1 3] / 4 along x, then along y, onto a plane of height x width."""
    return _up_axis(_up_axis(c, width, 1), height, 0)


def level_weights(L, spread):
    """w_1 .. w_L: p_1 = 1, p_k = p_{k-1} * (double)spread, S their sum in order, w_k = (float)(p_k / S)."""
    sp = float(f32(spread))
    p, total = [], 0.0
    for k in range(L):
        p.append(1.0 if k == 0 else p[-1] * sp)
        total = total + p[-1]
    return [f32(v / total) for v in p]


def glare(rgba, samples=1, levels=6, spread=1.0, strength=0.08, max_value=65536.0, planes=False):
    """-> the glared mean [h, w, 4] (alpha = the input's); with planes=True also the list A_1 .. A_L."""
    a = np.asarray(rgba, dtype=f32)
    h, w = a.shape[:2]
    s = sanitise(a, samples, max_value)
    L = effective_levels(levels, w, h)
    out = s.copy()
    A = []
    if L > 0:
        with np.errstate(all="ignore"):
            D = [s]
            for _ in range(L):
                D.append(down(D[-1]))
            wk = level_weights(L, spread)
            acc = D[L] * wk[L - 1]
            A = [acc]
            for k in range(L - 1, 0, -1):
                acc = D[k] * wk[k - 1] + up(acc, *D[k].shape[:2])
                A.insert(0, acc)
            G = up(acc, h, w)
            out = s + (G - s) * f32(strength)
    out = out.astype(f32)
    out[..., 3] = a[..., 3]
    return (out, A) if planes else out


def ulps(a, b):
    """The distance of two arrays of non-negative finite float32 in units of the last place."""
    return np.abs(np.asarray(a, dtype=f32).view(np.int32).astype(np.int64) - np.asarray(b, dtype=f32).view(np.int32).astype(np.int64))


def make_frame(width, height, seed=1, poison=True):
    """A log-normal frame of running sums over 2^-20 .. 2^20 (alpha 1 .. 2); with `poison` NaN, -3, -inf, +inf and 3e38 visit the
    first pixel, the last pixel and pixel 256 (where the frame has one)."""
    rng = np.random.default_rng(seed)
    a = np.exp2(np.clip(rng.normal(0.0, 6.0, size=(height, width, 4)), -20.0, 20.0)).astype(f32)
    a[..., 3] = rng.uniform(1.0, 2.0, size=(height, width)).astype(f32)
    if poison:
        flat = a.reshape(-1, 4)
        bad = [f32(np.nan), f32(-3.0), f32(-np.inf), f32(np.inf), f32(3e38)]
        for n, at in enumerate(p for p in (0, flat.shape[0] - 1, 256) if p < flat.shape[0]):
            for ch in range(3):
                flat[at, ch] = bad[(n + ch) % 5]
            if at + 1 < flat.shape[0]:
                flat[at + 1, 0] = bad[(n + 3) % 5]
                flat[at + 1, 1] = bad[(n + 4) % 5]
    return a
