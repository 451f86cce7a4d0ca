// bt_compare.hpp -- EXTENSION, NOT IN THE REFERENCE: the compare stage's definition, operation by operation (include/bendy_hip.h,
// bt_compare): how far a test frame X is from a reference frame Y -- MSE, relMSE, PSNR, SSIM, the largest
// difference, the share of the error that the worst pixels carry, and a false-colour error map.  Plain __host__ __device__ code
// without a HIP runtime call: the kernels (bt_compare.hip), the host entry point bt_debug_compare_host and
// tests/cpp/compare_check.cpp run the same lines, so the whole stage is tested on a machine without a GPU.  Builds with a plain
// C++ compiler too.  tests/compare_ref.py restates it in numpy.
//
// Everything is float64 unless marked float32, in the order written (-ffp-contract=off); only + - * /, max and compares appear.
// Both frames are w x h RGBA32F running sums with their counts n_x, n_y (a mean has count 1); alpha is ignored.
//
//   1. point      float32: r = 1 / n once per frame; x = X.rgb * r_x, y = Y.rgb * r_y.  The pixel is BAD if any of the six fails
//                 |v| < inf: it counts in `nonfinite`, is not in `valid`, and every term below is 0.  Else, widened to float64,
//                 per channel d = x - y, e = d d, q = e / (y y + epsilon); se = (e.r + e.g) + e.b, re = (q.r + q.g) + q.b,
//                 m = max(|d.r|, |d.g|, |d.b|).  The error plane, float32: E = re < FLT_MAX ? (float)re : FLT_MAX; a bad pixel
//                 holds -0.0f, which compares equal to 0 and whose sign bit keeps it out of the tail and paints it magenta.
//   2. structure  float32: Yf = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z on x and on y; Yc = Yf > 0 ? (Yf < FLT_MAX ? Yf : FLT_MAX)
//                 : 0 (a NaN fails the compare; a bad pixel holds 0 on both sides).  float64: v = Yc / (1 + Yc), in [0, 1] (1 from about 2^53 on).
//   3. SSIM       11 taps, sigma 1.5, the weights of weight() below as literals.  vx, vy, vx vx, vy vy, vx vy (the products formed first)
//                 are blurred along x, then along y, each as acc = 0; acc = acc + W[k] a[clamp(i + k - 5, 0, n - 1)], k = 0 .. 10.
//                 With mx, my, xx, yy, xy:  sx = xx - mx mx; sy = yy - my my; cxy = xy - mx my;
//                 s = ((2 (mx my) + C1) (2 cxy + C2)) / (((mx mx + my my) + C1) ((sx + sy) + C2)), C1 = 1e-4, C2 = 9e-4.
//   4. sums       per 16 x 16 tile, slot k = ly 16 + lx, 0.0 outside the frame: for stride = 128, 64 .. 1: t[k] = t[k] + t[k +
//                 stride], k < stride.  The tiles' t[0] are added one after another in tile order ty tiles_x + tx, from 0.0.
//   5. results    mse = S_se / (3 valid), rel_mse = S_re / (3 valid) (0 without a valid pixel), ssim = S_s / pixels, max_abs
//                 = max m and the smallest y w + x that attains it, psnr = 10 log10(peak peak / mse) on the host.
//   6. tail       k = clamp(ceil(fraction valid), 1, valid); T = the k-th largest E over the valid pixels, by a radix select
//                 over the bit patterns (11, 11 and 10 bits); c_gt = #(E > T), S_gt = the sum of (double)E over those, S_all over
//                 all valid ones, by step 4; share = (S_gt + (k - c_gt) (double)T) / S_all, 0 when S_all == 0.
//   7. map        float32: t = min(E / scale, 1); r = min(3 t, 1), g = clamp(3 t - 1, 0, 1), b = clamp(3 t - 2, 0, 1), each
//                 stored as (uint8)(v 255 + 0.5), alpha 255; a bad pixel is (255, 0, 255).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define BT_COMPARE_HD __host__ __device__ inline
#else
#define BT_COMPARE_HD inline
#endif

#define BT_COMPARE_TILE 16
#define BT_COMPARE_TAPS 11
#define BT_COMPARE_SPAN 26             // 16 outputs of an axis and five texels either side
#define BT_COMPARE_BINS 2048

namespace btcompare {

constexpr float kFltMax = 3.40282346638528859811704183484516925e+38f;
constexpr double kC1 = 1e-4, kC2 = 9e-4;

struct Texel {
    float x, y, z, w;
};
struct Pair {                          // (vx, vy) of one pixel
    double x, y;
};

// the window: exp(-(k - 5)^2 / 4.5) normalised, rounded once to float64 and kept as literals.  A chain of compares, not a table:
// with the taps unrolled every call folds to its constant and no array is indexed by a variable.
BT_COMPARE_HD double weight(int k) {
    const int j = k > 5 ? 10 - k : k;
    return j == 0 ? 0x1.0d956b52a1d70p-10
         : j == 1 ? 0x1.f1fe01ae5a5b8p-8
         : j == 2 ? 0x1.26eb175d83f67p-5
         : j == 3 ? 0x1.bff0fe8e98418p-4
         : j == 4 ? 0x1.b43c3f52b19f2p-3
                  : 0x1.106560aa892c0p-2;
}

BT_COMPARE_HD uint32_t clamp_index(int64_t i, uint32_t n) { return i < 0 ? 0u : i > (int64_t)n - 1 ? n - 1u : (uint32_t)i; }
// texel of entry `a` of a tile's staged axis, the tile starting at pixel i0: the staging clamps, so that no address outside a
// plane is formed, and tap k of pixel i0 + l is entry l + k
BT_COMPARE_HD uint32_t stage_texel(uint32_t i0, uint32_t a, uint32_t n) { return clamp_index((int64_t)i0 + (int64_t)a - 5, n); }

BT_COMPARE_HD bool finite32(float v) { return (v < 0.0f ? -v : v) < __builtin_huge_valf(); }
BT_COMPARE_HD double abs64(double v) { return v < 0.0 ? -v : v; }
BT_COMPARE_HD uint32_t bits_of(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
}

// ---- steps 1 and 2 ----
struct Point {
    double se, re, m;
    float E;
    Pair v;
    bool bad;
};
BT_COMPARE_HD float luminance(float x, float y, float z) {
    const float Yf = (0.2126f * x + 0.7152f * y) + 0.0722f * z;
    return Yf > 0.0f ? (Yf < kFltMax ? Yf : kFltMax) : 0.0f;
}
BT_COMPARE_HD double compress(float Yc) { return (double)Yc / (1.0 + (double)Yc); }
BT_COMPARE_HD void channel(float x, float y, double epsilon, double &d, double &e, double &q) {
    d = (double)x - (double)y;
    e = d * d;
    q = e / ((double)y * (double)y + epsilon);
}
template <class T>
BT_COMPARE_HD Point point(T X, float rx, T Y, float ry, double epsilon) {
    const float x0 = X.x * rx, x1 = X.y * rx, x2 = X.z * rx, y0 = Y.x * ry, y1 = Y.y * ry, y2 = Y.z * ry;
    Point p;
    p.bad = !(finite32(x0) && finite32(x1) && finite32(x2) && finite32(y0) && finite32(y1) && finite32(y2));
    if (p.bad) {
        p.se = p.re = p.m = 0.0;
        p.E = -0.0f;
        p.v.x = p.v.y = compress(0.0f);
        return p;
    }
    double d0, d1, d2, e0, e1, e2, q0, q1, q2;
    channel(x0, y0, epsilon, d0, e0, q0);
    channel(x1, y1, epsilon, d1, e1, q1);
    channel(x2, y2, epsilon, d2, e2, q2);
    p.se = (e0 + e1) + e2;
    p.re = (q0 + q1) + q2;
    const double a0 = abs64(d0), a1 = abs64(d1), a2 = abs64(d2), a01 = a0 > a1 ? a0 : a1;
    p.m = a01 > a2 ? a01 : a2;
    p.E = p.re < (double)kFltMax ? (float)p.re : kFltMax;
    p.v.x = compress(luminance(x0, x1, x2));
    p.v.y = compress(luminance(y0, y1, y2));
    return p;
}

// ---- step 3 ----
struct Five {
    double mx, my, xx, yy, xy;
};
BT_COMPARE_HD Five five_zero() { return Five{0.0, 0.0, 0.0, 0.0, 0.0}; }
// one tap of the first (x) blur: the products are formed from the texel, then weighed
BT_COMPARE_HD void tap_pair(Five &acc, double w, Pair v) {
    acc.mx = acc.mx + w * v.x;
    acc.my = acc.my + w * v.y;
    acc.xx = acc.xx + w * (v.x * v.x);
    acc.yy = acc.yy + w * (v.y * v.y);
    acc.xy = acc.xy + w * (v.x * v.y);
}
// one tap of the second (y) blur
BT_COMPARE_HD void tap_five(Five &acc, double w, const Five &a) {
    acc.mx = acc.mx + w * a.mx;
    acc.my = acc.my + w * a.my;
    acc.xx = acc.xx + w * a.xx;
    acc.yy = acc.yy + w * a.yy;
    acc.xy = acc.xy + w * a.xy;
}
BT_COMPARE_HD double ssim_of(const Five &b) {
    const double sx = b.xx - b.mx * b.mx, sy = b.yy - b.my * b.my, cxy = b.xy - b.mx * b.my;
    return ((2.0 * (b.mx * b.my) + kC1) * (2.0 * cxy + kC2)) / (((b.mx * b.mx + b.my * b.my) + kC1) * ((sx + sy) + kC2));
}

// ---- step 4 ----
// (m, index): the larger m, and of equal ones the smaller index
BT_COMPARE_HD void max_merge(double &m, uint32_t &index, double m2, uint32_t index2) {
    if (m2 > m || (m2 == m && index2 < index)) {
        m = m2;
        index = index2;
    }
}
// the tile's tree, as written
inline double tile_tree(double *t) {
    for (uint32_t stride = 128; stride >= 1; stride >>= 1)
        for (uint32_t k = 0; k < stride; ++k) t[k] = t[k] + t[k + stride];
    return t[0];
}
inline double ordered_sum(const double *p, size_t n) {
    double s = 0.0;
    for (size_t i = 0; i < n; ++i) s = s + p[i];
    return s;
}

// ---- step 6 ----
// A pass of the radix select looks at the valid pixels whose bits above `prefix_shift` equal `prefix`, and bins the bits
// [shift, prefix_shift).  The passes are (21, 31, 0), (10, 21, b1), (0, 10, b1 b2): a bad pixel's sign bit fails the first.
BT_COMPARE_HD bool in_pass(uint32_t u, uint32_t prefix_shift, uint32_t prefix) { return (u >> prefix_shift) == prefix; }
BT_COMPARE_HD uint32_t bin_of(uint32_t u, uint32_t shift, uint32_t prefix_shift) { return (u >> shift) & ((1u << (prefix_shift - shift)) - 1u); }
constexpr uint32_t kPassShift[3] = {21, 10, 0}, kPassPrefixShift[3] = {31, 21, 10};
// the bin that holds the k-th largest (k >= 1) of the pass; k becomes its rank inside that bin
inline uint32_t select_bin(const uint32_t *hist, uint64_t &k) {
    for (uint32_t b = BT_COMPARE_BINS; b-- > 0;) {
        if (hist[b] >= k) return b;
        k -= hist[b];
    }
    return 0;                          // not reached while k <= the pass's count
}
inline uint64_t tail_rank(double fraction, uint64_t valid) {
    const double want = fraction * (double)valid;
    uint64_t k = (uint64_t)want;
    if ((double)k < want) ++k;         // ceil
    return k < 1 ? 1 : k > valid ? valid : k;
}
struct TailTerm {
    double gt, all;
    uint32_t c_gt;
};
BT_COMPARE_HD TailTerm tail_term(float E, float T) {
    TailTerm t{0.0, 0.0, 0u};
    if (bits_of(E) >> 31) return t;    // a bad pixel
    t.all = (double)E;
    if (E > T) {
        t.gt = (double)E;
        t.c_gt = 1u;
    }
    return t;
}
inline double tail_share(double S_gt, double S_all, uint64_t c_gt, uint64_t k, float T) {
    if (S_all == 0.0) return 0.0;
    return (S_gt + (double)(k - c_gt) * (double)T) / S_all;
}

// ---- step 7 ----
BT_COMPARE_HD float clamp01(float v) { return v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f; }
BT_COMPARE_HD uint32_t map_pixel(float E, float scale) {                  // r | g << 8 | b << 16 | a << 24
    if (bits_of(E) >> 31) return 0xffff00ffu;
    const float q = E / scale, t = q < 1.0f ? q : 1.0f, t3 = 3.0f * t;
    const float r = t3 < 1.0f ? t3 : 1.0f, g = clamp01(t3 - 1.0f), b = clamp01(t3 - 2.0f);
    const uint32_t R = (uint32_t)(uint8_t)(r * 255.0f + 0.5f), G = (uint32_t)(uint8_t)(g * 255.0f + 0.5f), B = (uint32_t)(uint8_t)(b * 255.0f + 0.5f);
    return R | (G << 8) | (B << 16) | 0xff000000u;
}

// ---- the frame sums and what step 5 makes of them ----
struct Sums {
    double se = 0.0, re = 0.0, s = 0.0, max_abs = 0.0;
    uint64_t valid = 0, nonfinite = 0, pixels = 0;
    uint32_t max_index = 0;
};
inline uint32_t tiles_of(uint32_t side) { return side / BT_COMPARE_TILE + (side % BT_COMPARE_TILE != 0u); }

// The whole of steps 1 .. 4 on the host, single-threaded.  E: w h floats, V: w h pairs, S: w h doubles.
inline void run_host(const Texel *X, uint32_t nx, const Texel *Y, uint32_t ny, uint32_t w, uint32_t h, double epsilon, float *E, Pair *V,
                     double *S, Sums &out) {
    const float rx = 1.0f / (float)nx, ry = 1.0f / (float)ny;
    const uint32_t tx_n = tiles_of(w), ty_n = tiles_of(h);
    out = Sums();
    out.pixels = (uint64_t)w * h;
    out.max_index = 0xffffffffu;       // above every pixel's index: the first tile's pair replaces it
    double t_se[256], t_re[256], t_s[256];
    // steps 1 and 2, tile by tile
    for (uint32_t ty = 0; ty < ty_n; ++ty)
        for (uint32_t tx = 0; tx < tx_n; ++tx) {
            double m = 0.0;
            uint32_t index = 0xffffffffu;
            for (uint32_t k = 0; k < 256; ++k) {
                const uint32_t i = tx * BT_COMPARE_TILE + k % BT_COMPARE_TILE, j = ty * BT_COMPARE_TILE + k / BT_COMPARE_TILE;
                t_se[k] = t_re[k] = 0.0;
                if (i >= w || j >= h) continue;
                const size_t p = (size_t)j * w + i;
                const Point pt = point(X[p], rx, Y[p], ry, epsilon);
                E[p] = pt.E;
                V[p] = pt.v;
                t_se[k] = pt.se;
                t_re[k] = pt.re;
                if (pt.bad) ++out.nonfinite;
                else ++out.valid;
                max_merge(m, index, pt.m, (uint32_t)p);
            }
            out.se = out.se + tile_tree(t_se);
            out.re = out.re + tile_tree(t_re);
            max_merge(out.max_abs, out.max_index, m, index);
        }
    // step 3, tile by tile through a stage and a row-blurred stage, as the kernel does
    Pair stage[BT_COMPARE_SPAN * BT_COMPARE_SPAN];
    Five rows[BT_COMPARE_SPAN * BT_COMPARE_TILE];
    for (uint32_t ty = 0; ty < ty_n; ++ty)
        for (uint32_t tx = 0; tx < tx_n; ++tx) {
            const uint32_t i0 = tx * BT_COMPARE_TILE, j0 = ty * BT_COMPARE_TILE;
            for (uint32_t b = 0; b < BT_COMPARE_SPAN; ++b)
                for (uint32_t a = 0; a < BT_COMPARE_SPAN; ++a)
                    stage[b * BT_COMPARE_SPAN + a] = V[(size_t)stage_texel(j0, b, h) * w + stage_texel(i0, a, w)];
            for (uint32_t b = 0; b < BT_COMPARE_SPAN; ++b)
                for (uint32_t lx = 0; lx < BT_COMPARE_TILE; ++lx) {
                    Five acc = five_zero();
                    for (int k = 0; k < BT_COMPARE_TAPS; ++k) tap_pair(acc, weight(k), stage[b * BT_COMPARE_SPAN + lx + k]);
                    rows[b * BT_COMPARE_TILE + lx] = acc;
                }
            for (uint32_t k = 0; k < 256; ++k) {
                const uint32_t lx = k % BT_COMPARE_TILE, ly = k / BT_COMPARE_TILE, i = i0 + lx, j = j0 + ly;
                t_s[k] = 0.0;
                if (i >= w || j >= h) continue;
                Five acc = five_zero();
                for (int t = 0; t < BT_COMPARE_TAPS; ++t) tap_five(acc, weight(t), rows[(ly + t) * BT_COMPARE_TILE + lx]);
                const double s = ssim_of(acc);
                S[(size_t)j * w + i] = s;
                t_s[k] = s;
            }
            out.s = out.s + tile_tree(t_s);
        }
}

// Step 6 on the host over the plane E: the three histogram passes, then the three sums by step 4.
inline void tail_host(const float *E, uint32_t w, uint32_t h, uint64_t valid, double fraction, double &share, float &threshold) {
    share = 0.0;
    threshold = 0.0f;
    if (valid == 0) return;
    const uint64_t k0 = tail_rank(fraction, valid);
    uint64_t k = k0;
    const size_t n = (size_t)w * h;
    uint32_t prefix = 0;
    uint32_t *hist = new uint32_t[BT_COMPARE_BINS];
    for (int pass = 0; pass < 3; ++pass) {
        for (uint32_t b = 0; b < BT_COMPARE_BINS; ++b) hist[b] = 0;
        for (size_t p = 0; p < n; ++p) {
            const uint32_t u = bits_of(E[p]);
            if (in_pass(u, kPassPrefixShift[pass], prefix)) ++hist[bin_of(u, kPassShift[pass], kPassPrefixShift[pass])];
        }
        const uint32_t b = select_bin(hist, k);
        prefix = (prefix << (kPassPrefixShift[pass] - kPassShift[pass])) | b;
    }
    delete[] hist;
    memcpy(&threshold, &prefix, 4);
    const uint32_t tx_n = tiles_of(w), ty_n = tiles_of(h);
    double t_gt[256], t_all[256], S_gt = 0.0, S_all = 0.0;
    uint64_t c_gt = 0;
    for (uint32_t ty = 0; ty < ty_n; ++ty)
        for (uint32_t tx = 0; tx < tx_n; ++tx) {
            for (uint32_t q = 0; q < 256; ++q) {
                const uint32_t i = tx * BT_COMPARE_TILE + q % BT_COMPARE_TILE, j = ty * BT_COMPARE_TILE + q / BT_COMPARE_TILE;
                t_gt[q] = t_all[q] = 0.0;
                if (i >= w || j >= h) continue;
                const TailTerm t = tail_term(E[(size_t)j * w + i], threshold);
                t_gt[q] = t.gt;
                t_all[q] = t.all;
                c_gt += t.c_gt;
            }
            S_gt = S_gt + tile_tree(t_gt);
            S_all = S_all + tile_tree(t_all);
        }
    share = tail_share(S_gt, S_all, c_gt, k0, threshold);
}

} // namespace btcompare

// ---- the launchers of bt_compare.hip (for the translation units that include <hip/hip_runtime.h> and define
// BT_COMPARE_LAUNCHERS first).  hipErrorInvalidConfiguration for a frame whose tiles do not fit one launch. ----
#ifdef BT_COMPARE_LAUNCHERS
// One slot per tile, structure of arrays in one allocation of `tiles` * BT_COMPARE_SLAB_BYTES bytes: the doubles first.
#define BT_COMPARE_SLAB_BYTES 64
struct BtCompareSlab {
    double *se, *re, *s, *m, *gt, *all;
    uint32_t *valid, *nonfinite, *index, *c_gt;
};
inline BtCompareSlab bt_compare_slab(void *mem, size_t tiles) {
    BtCompareSlab b;
    double *d = (double *)mem;
    b.se = d;
    b.re = d + tiles;
    b.s = d + 2 * tiles;
    b.m = d + 3 * tiles;
    b.gt = d + 4 * tiles;
    b.all = d + 5 * tiles;
    uint32_t *u = (uint32_t *)(d + 6 * tiles);
    b.valid = u;
    b.nonfinite = u + tiles;
    b.index = u + 2 * tiles;
    b.c_gt = u + 3 * tiles;
    return b;
}
extern "C" {
hipError_t bt_launch_compare_point(const float *X, float rx, const float *Y, float ry, uint32_t w, uint32_t h, double epsilon, float *E,
                                   double *V, BtCompareSlab slab, hipStream_t stream);
hipError_t bt_launch_compare_ssim(const double *V, uint32_t w, uint32_t h, double *S, BtCompareSlab slab, hipStream_t stream);
hipError_t bt_launch_compare_hist(const float *E, uint32_t n, uint32_t shift, uint32_t prefix_shift, uint32_t prefix, uint32_t *hist,
                                  hipStream_t stream);
hipError_t bt_launch_compare_tail(const float *E, uint32_t w, uint32_t h, float T, BtCompareSlab slab, hipStream_t stream);
hipError_t bt_launch_compare_map(const float *E, uint32_t n, float scale, uint8_t *rgba8, hipStream_t stream);
}
#endif
