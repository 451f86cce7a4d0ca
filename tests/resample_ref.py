"""numpy restatement of the resample stage (EXTENSION; include/bendy_hip.h bt_resample): sanitise, the per-axis
weight tables, the horizontal and the vertical pass, the clamp and the alpha, operation by operation in the order
csrc/bt_resample.hpp has them.  Every float32 step is one correctly rounded numpy float32 operation on whole planes; the tables
are Python floats (IEEE float64) through + - * / alone, except lanczos3's two sines, and are rounded once to float32."""
import math

import numpy as np

from glare_ref import make_frame, sanitise, ulps  # noqa: F401  (step 1 is the glare stage's; the frames and ulps are shared)

f32 = np.float32

BOX, TENT, MITCHELL, LANCZOS3 = 0, 1, 2, 3
FILTERS = {"box": BOX, "tent": TENT, "mitchell": MITCHELL, "lanczos3": LANCZOS3}
RADIUS = {BOX: 0.5, TENT: 1.0, MITCHELL: 2.0, LANCZOS3: 3.0}
MAX_TAPS = 128
# bt_resample_params_default
DEFAULTS = dict(filter=MITCHELL, max_value=65536.0, clamp_negative=1)


def kernel(filt, x):
    """k(x) in float64; 0 outside the support."""
    a = -x if x < 0.0 else x
    if filt == BOX:
        return 1.0 if -0.5 <= x < 0.5 else 0.0
    if filt == TENT:
        return 1.0 - a if a < 1.0 else 0.0
    if filt == MITCHELL:
        if a < 1.0:
            return (((21.0 * a - 36.0) * a) * a + 16.0) / 18.0
        if a < 2.0:
            return (((-7.0 * a + 36.0) * a - 60.0) * a + 32.0) / 18.0
        return 0.0
    if x == 0.0:
        return 1.0
    if a >= 3.0 or x == float(round(x)):               # exactly 0 at every other integer
        return 0.0
    p = math.pi * x
    q = p / 3.0
    return (math.sin(p) / p) * (math.sin(q) / q)


def axis_table(src, dst, filt):
    """-> (first int64 [dst] unclamped, T, weights float32 [dst, T] padded with 0, nearest int64 [dst])."""
    ratio = float(src) / float(dst)
    s = ratio if ratio > 1.0 else 1.0
    reach = RADIUS[filt] * s
    rows, first, nearest = [], [], []
    for i in range(dst):
        c = (float(i) + 0.5) * ratio - 0.5
        lo, hi = math.ceil(c - reach), math.floor(c + reach)
        k = [kernel(filt, (float(j) - c) / s) for j in range(lo, hi + 1)]
        total = 0.0
        for v in k:
            total = total + v
        rows.append([f32(v / total) for v in k])
        first.append(lo)
        nearest.append(min(src - 1, math.floor((float(i) + 0.5) * ratio)))
    T = max(len(r) for r in rows)
    w = np.zeros((dst, T), dtype=f32)
    for i, r in enumerate(rows):
        w[i, :len(r)] = r
    return np.array(first, dtype=np.int64), T, w, np.array(nearest, dtype=np.int64)


def _pass(p, table, axis):
    """acc = 0; acc = acc + w * v over all T taps in ascending order, the taps clamped to the plane."""
    first, T, w, _ = table
    first = np.asarray(first, dtype=np.int64)
    side = p.shape[axis]
    shape = [1, 1, 1]
    shape[axis] = len(first)
    acc = None
    with np.errstate(all="ignore"):
        for t in range(T):
            v = np.take(p, np.clip(first + t, 0, side - 1), axis=axis)
            prod = (w[:, t].astype(f32).reshape(shape) * v).astype(f32)
            acc = (np.zeros_like(prod) + prod) if acc is None else acc + prod
    return acc.astype(f32)


def resample(rgba, samples, width, height, filter=MITCHELL, max_value=65536.0, clamp_negative=1, tables=None, plane=False):
    """-> the resampled mean [height, width, 4] (alpha = the input's at the nearest pixel); with plane=True also P [h, width, 4].
    `tables`: (x table, y table) as axis_table returns them -- the library's own, or None for this module's."""
    a = np.asarray(rgba, dtype=f32)
    h, w = a.shape[:2]
    filt = FILTERS.get(filter, filter) if isinstance(filter, str) else int(filter)
    tx, ty = tables if tables is not None else (axis_table(w, width, filt), axis_table(h, height, filt))
    s = sanitise(a, samples, max_value)
    P = _pass(s, tx, 1)
    acc = _pass(P, ty, 0)
    with np.errstate(all="ignore"):
        out = np.where(acc >= 0, acc, f32(0.0)).astype(f32) if clamp_negative else acc.copy()
    out[..., 3] = a[np.asarray(ty[3], dtype=np.int64)[:, None], np.asarray(tx[3], dtype=np.int64)[None, :], 3]
    return (out, P) if plane else out
