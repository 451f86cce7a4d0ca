"""numpy restatement of the adaptive sampler's arithmetic (EXTENSION; test infrastructure).

Y, M and e_p are float32, elementwise, in the order include/bendy_hip.h states them (numpy rounds every float32 operation
correctly, as the kernels' `/` and sqrt do, and fuses nothing).  The tile mean and the decision are float64: the kernel's
float32 reduction in whatever order is compared against them with a margin (tests/test_gpu_adaptive.py)."""
import numpy as np

F = np.float32
BT_TILE = 16
KR, KG, KB = F(0.2126), F(0.7152), F(0.0722)


def luminance(rgb):
    """Y = (0.2126 r + 0.7152 g) + 0.0722 b, float32."""
    rgb = np.asarray(rgb, dtype=F)
    return (KR * rgb[..., 0] + KG * rgb[..., 1]) + KB * rgb[..., 2]


def moment_of(samples):
    """samples: float32 [T, ..., 3] in sample order -> M = ((0 + Y0*Y0) + Y1*Y1) + ..., float32."""
    return moment_add(np.zeros(np.asarray(samples).shape[1:-1], dtype=F), samples)


def moment_add(m, samples):
    """Continues the plane `m` with more samples."""
    m = np.array(m, dtype=F, copy=True)
    for s in np.asarray(samples, dtype=F):
        y = luminance(s)
        m = m + y * y
    return m


def pixel_error(sums_rgb, moment, count, eps):
    """e_p per pixel, float32; `count` a scalar or an array broadcastable to the pixels (0 gives 0: nothing sampled)."""
    c = np.asarray(count).astype(F)
    with np.errstate(all="ignore"):
        S = luminance(sums_rgb)
        mu = S / c
        var = np.maximum(F(0), np.asarray(moment, dtype=F) / c - mu * mu)
        ep = np.sqrt(var / c) / (mu + F(eps))
    return np.where(np.isfinite(ep), ep, F(0)).astype(F)


def tile_shape(width, height):
    return (height + BT_TILE - 1) // BT_TILE, (width + BT_TILE - 1) // BT_TILE


def per_pixel(tiles, width, height):
    """[tiles_y, tiles_x] -> [height, width]: each pixel's tile's value."""
    return np.repeat(np.repeat(np.asarray(tiles), BT_TILE, axis=0), BT_TILE, axis=1)[:height, :width]


def tile_error(sums, moment, counts, eps=1e-3):
    """e_t per tile in float64: the mean of the float32 e_p over the tile's pixels inside the frame.
    sums [H, W, >= 3], moment [H, W], counts [tiles_y, tiles_x] (the counts the errors are for)."""
    h, w = moment.shape
    ty, tx = tile_shape(w, h)
    out = np.zeros((ty, tx), dtype=np.float64)
    ep = pixel_error(sums[..., :3], moment, per_pixel(counts, w, h), eps).astype(np.float64)
    for j in range(ty):
        for i in range(tx):
            blk = ep[j * BT_TILE:(j + 1) * BT_TILE, i * BT_TILE:(i + 1) * BT_TILE]
            out[j, i] = blk.sum() / blk.size
    return out


def goes_on(count, e_t, threshold, min_samples, max_samples):
    """The decision for tiles with count `count` (after the pass) and error e_t: True = still active."""
    count = np.asarray(count)
    return ~((count >= max_samples) | ((count >= min_samples) & (np.asarray(e_t, dtype=np.float64) <= float(F(threshold)))))
