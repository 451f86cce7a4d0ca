"""numpy restatement of the despeckle stage (EXTENSION; include/bendy_hip.h bt_despeckle): sanitise, luminance, the
k-th largest luminance of the in-frame neighbours, the limit and the pull-down, operation by operation in the order
csrc/bt_despeckle.hpp has them.  Every float32 step is one correctly rounded numpy float32 operation on whole planes.  The order
statistic is taken by sorting: its value does not depend on how it is selected."""
import numpy as np

f32 = np.float32

# bt_despeckle_params_default
DEFAULTS = dict(radius=1, rank=2, ratio=4.0, floor=0.01, max_value=65536.0)


def max_rank(radius):
    return (2 * radius + 1) ** 2 - 1


def sanitise(rgba, samples, max_value):
    """cap = max_value * (float)n;  s = v >= 0 ? v : 0;  s = s < cap ? s : cap  ->  (s [h, w, 3], changed [h, w])."""
    v = np.asarray(rgba, dtype=f32)[..., :3]
    cap = f32(max_value) * f32(samples)
    with np.errstate(all="ignore"):
        s = np.where(v >= 0, v, f32(0.0)).astype(f32)
        s = np.where(s < cap, s, cap).astype(f32)
        changed = (~(s == v)).any(axis=-1)
    return s, changed


def luminance(s):
    """Y = (0.2126 x + 0.7152 y) + 0.0722 z, the display meter's weights and parenthesisation."""
    with np.errstate(all="ignore"):
        return ((f32(0.2126) * s[..., 0] + f32(0.7152) * s[..., 1]) + f32(0.0722) * s[..., 2]).astype(f32)


def neighbour_count(width, height, radius):
    """M [h, w]: the in-frame pixels of the (2 radius + 1)^2 window, centre excluded."""
    x, y = np.arange(width, dtype=np.int64), np.arange(height, dtype=np.int64)
    nx = np.minimum(x + radius, width - 1) - np.maximum(x - radius, 0) + 1
    ny = np.minimum(y + radius, height - 1) - np.maximum(y - radius, 0) + 1
    return ny[:, None] * nx[None, :] - 1


def kth_largest(Y, radius, rank):
    """(T [h, w], M [h, w]): the min(rank, M)-th largest Y among each pixel's in-frame neighbours; T is 0 where M = 0."""
    h, w = Y.shape
    R = int(radius)
    padded = np.full((h + 2 * R, w + 2 * R), f32(-1.0), dtype=f32)        # absent taps sort below every luminance
    padded[R:R + h, R:R + w] = Y
    taps = [padded[R + dy:R + dy + h, R + dx:R + dx + w] for dy in range(-R, R + 1) for dx in range(-R, R + 1) if (dx, dy) != (0, 0)]
    ordered = -np.sort(-np.stack(taps), axis=0)                            # descending
    M = neighbour_count(w, h, R)
    k = np.minimum(int(rank), M)
    T = np.take_along_axis(ordered, np.maximum(k - 1, 0)[None], axis=0)[0]
    return np.where(M > 0, T, f32(0.0)).astype(f32), M


def despeckle(rgba, samples=1, radius=1, rank=2, ratio=4.0, floor=0.01, max_value=65536.0, details=False):
    """-> the despeckled sums [h, w, 4] (alpha = the input's); with details=True also a dict of flagged [h, w], sanitised
    [h, w], Y, lim and the counts."""
    a = np.asarray(rgba, dtype=f32)
    s, changed = sanitise(a, samples, max_value)
    Y = luminance(s)
    T, M = kth_largest(Y, radius, rank)
    fl = f32(floor) * f32(samples)
    with np.errstate(all="ignore"):
        lim = (T * f32(ratio) + fl).astype(f32)
        flagged = (M > 0) & (Y > lim)
        g = np.where(flagged, lim / np.where(flagged, Y, f32(1.0)), f32(1.0)).astype(f32)
        rgb = np.where(flagged[..., None], s * g[..., None], s).astype(f32)
    out = np.concatenate([rgb, a[..., 3:4]], axis=-1)
    if details:
        return out, dict(flagged=flagged, sanitised=changed, Y=Y, lim=lim, counts=(int(flagged.sum()), int(changed.sum()), int(Y.size)))
    return out


def counts(rgba, samples=1, **params):
    """(flagged, sanitised, pixels), as bt_despeckle_poll returns them."""
    return despeckle(rgba, samples, details=True, **{**DEFAULTS, **params})[1]["counts"]


def ramp(width, height):
    """1 + x / 32 + y / 16 in all three channels, alpha 1: a frame the defaults flag nothing of."""
    x, y = np.meshgrid(np.arange(width, dtype=f32), np.arange(height, dtype=f32))
    v = (f32(1.0) + x / f32(32.0) + y / f32(16.0)).astype(f32)
    return np.stack([v, v, v, np.ones_like(v)], axis=-1)
