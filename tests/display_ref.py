"""numpy restatement of the display stage (EXTENSION; include/bendy_hip.h bt_display): meter, expose and the tone
operators, operation by operation in the order csrc/bt_display.hip has them.  Every float32 step is one correctly rounded numpy
float32 operation; the counts are integers, so the histogram is independent of the order of summation; the mean of the bin
centres and log2(key) are float64 (the key is a double in bt_display_params).  exp2_bt is bt_color.hpp's polynomial with each fused multiply-add formed in float64 (the
product of two float32 is exact there) and rounded once more to float32, which can differ from the device's single rounding in
the last bit: the GPU tests therefore take `mult` from the device and check it against 2^e separately."""
import math

import numpy as np

f32 = np.float32

BINS = 256
Y_MIN, Y_MAX = f32(2.0 ** -16), f32(2.0 ** 16)
CLIP, REINHARD, ACES = 0, 1, 2

# bt_display_params_default
DEFAULTS = dict(key=0.18, tonemap=ACES, auto_exposure=1, ev=0.0, p_low=0.10, p_high=0.02, adapt=1.0, ev_min=-8.0, ev_max=8.0,
                white=4.0)


def luminance(rgba, samples):
    """c = rgb * (1 / n), Y = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z, in float32."""
    a = np.asarray(rgba, dtype=f32).reshape(-1, 4)
    r = f32(1.0) / f32(samples)
    with np.errstate(all="ignore"):
        c = a[:, :3] * r
        return (f32(0.2126) * c[:, 0] + f32(0.7152) * c[:, 1]) + f32(0.0722) * c[:, 2]


def pixel_with_luminance(y):
    """An RGBA pixel (alpha 1, samples = 1) whose float32 luminance is exactly `y`, a positive finite float32: one channel
    carries it, searched among the neighbours of y / weight (a channel's products are not dense in every binade, so the three
    channels are tried in turn)."""
    y = f32(y)
    for ch, wgt in ((1, 0.7152), (0, 0.2126), (2, 0.0722)):
        v = f32(y / f32(wgt))
        for cand in [v] + [fn(v, k) for k in range(1, 5) for fn in (_up, _down)]:
            px = np.array([[0, 0, 0, 1]], dtype=f32)
            px[0, ch] = cand
            if luminance(px, 1)[0] == y:
                return px[0]
    raise ValueError(f"no single-channel pixel has luminance {y!r}")


def _up(v, k):
    for _ in range(k):
        v = np.nextafter(v, f32(np.inf))
    return v


def _down(v, k):
    for _ in range(k):
        v = np.nextafter(v, f32(-np.inf))
    return v


def meter(rgba, samples):
    """-> (uint32[256] counts, under, over)."""
    y = luminance(rgba, samples)
    with np.errstate(invalid="ignore"):
        under = ~(y >= Y_MIN)                      # zero, negatives and NaN
        over = ~under & (y >= Y_MAX)               # +inf included
    inside = ~under & ~over
    bins = (y[inside].view(np.uint32) >> np.uint32(20)).astype(np.int64) - 888
    assert bins.size == 0 or (bins.min() >= 0 and bins.max() < BINS)
    return np.bincount(bins, minlength=BINS).astype(np.uint32), int(under.sum()), int(over.sum())


def target(hist, p):
    """The clamped exposure the histogram asks for, float32, or None for a frame without a pixel in range (W == 0)."""
    h = [int(v) for v in np.asarray(hist).reshape(BINS)]
    n = sum(h)
    lo = math.floor(float(f32(p["p_low"])) * n)
    hi = n - math.floor(float(f32(p["p_high"])) * n)
    P = W = S = 0
    for b in range(BINS):
        w = max(0, min(P + h[b], hi) - max(P, lo))
        W += w
        S += w * (2 * b + 1)
        P += h[b]
    if W == 0:
        return None
    m = S / (16.0 * W) - 16.0                      # float64: the mean of the bin centres in log2
    t = f32(math.log2(float(p["key"])) - m) + f32(p["ev"])
    return min(max(t, f32(p["ev_min"])), f32(p["ev_max"]))


def adapt_step(state, t, adapt):
    """state = (e, valid) -> the new state after a frame whose target is t (None: the state is left alone)."""
    e, valid = state
    if t is None:
        return state
    if not valid or f32(adapt) >= f32(1.0):
        return (f32(t), True)
    return (f32(e) + (f32(t) - f32(e)) * f32(adapt), True)


def shown_ev(state, p):
    """The exposure a frame is shown with under auto-exposure: the state's, or params.ev while there is none."""
    return f32(state[0]) if state[1] else f32(p["ev"])


def _fma(a, b, c):
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def exp2_bt(y):
    y = f32(y)
    k = f32(np.rint(y))
    z = (y - k) * f32(0.6931471805599453)
    p = _fma(z, f32(1.984126984e-4), f32(1.388888889e-3))
    for c in (8.333333333e-3, 4.166666667e-2, 1.666666667e-1, 0.5, 1.0, 1.0):
        p = _fma(p, z, f32(c))
    ki = int(k)
    if ki < -126:
        return f32(0.0)
    if ki > 127:
        return f32(np.inf)
    return p * f32(2.0 ** ki)


def tone(c, mult, op, white=4.0):
    """c: float32 [..., 3] means; x = c * mult, then the operator per channel, all float32."""
    with np.errstate(all="ignore"):
        x = np.asarray(c, dtype=f32) * f32(mult)
        if op == CLIP:
            return x
        x = np.where(x > 0, x, f32(0.0)).astype(f32)          # NaN and negatives -> 0
        one = f32(1.0)
        if op == REINHARD:
            iw2 = one / (f32(white) * f32(white))
            return (x * (one + x * iw2)) / (one + x)
        if op == ACES:                                         # Narkowicz's fit
            return (x * (f32(2.51) * x + f32(0.03))) / (x * (f32(2.43) * x + f32(0.59)) + f32(0.14))
    raise ValueError(op)


def shown_frame(rgba, samples, mult, op, white=4.0):
    """The RGBA32F mean frame whose plain preview (samples = 1) is what bt_show_kernel writes: rgb = tone(c * mult), a = a."""
    a = np.asarray(rgba, dtype=f32)
    with np.errstate(all="ignore"):
        c = a[..., :3] * (f32(1.0) / f32(samples))
    return np.concatenate([tone(c, mult, op, white), a[..., 3:]], axis=-1).astype(f32)
