// bt_resample.hpp -- EXTENSION, NOT IN THE REFERENCE: the resample stage's definition, texel by texel (include/bendy_hip.h,
// bt_resample).  Plain __host__ __device__ code without a HIP runtime call: the kernels (bt_resample.hip), the host
// entry point bt_debug_resample_host and tests/cpp/resample_check.cpp run the same lines, so the whole stage is tested on a
// machine without a GPU.  Builds with a plain C++ compiler too.  tests/resample_ref.py restates it in numpy.
//
// Pixels are float32 in the order written (-ffp-contract=off, correctly rounded division); the weight tables are float64 on the
// host, rounded once to float32.  A texel type T is any struct of four floats x, y, z, w; `fetch(p)` returns the texel at the
// (already clamped) position p of the axis that is filtered.  The input is w x h running sums of n samples, the output a W x H mean.
//
//   1. sanitise   bt_glare.hpp's step 1, the same function: r = 1 / n;  c = rgb * r;  s = c >= 0 ? c : 0;  s = s < max_value ? s :
//                 max_value;  s.w = 0.  It happens before any tap, so a NaN does not spread over a footprint.
//   2. tables     per axis (src -> dst texels, filter), on the host in float64:
//                     ratio = (double)src / dst;  s = ratio > 1 ? ratio : 1;  c_i = (i + 0.5) * ratio - 0.5
//                     first_i = ceil(c_i - R * s),  last_i = floor(c_i + R * s)       R = 0.5, 1, 2, 3 for box, tent, mitchell, lanczos3
//                     k_j = k((j - c_i) / s)  for j = first_i .. last_i;  S = their sum in ascending j;  w_ij = (float)(k_j / S)
//                     T = the largest last_i - first_i + 1 of the axis; every row is padded with weights 0 to T taps
//                     nearest_i = min(src - 1, floor((i + 0.5) * ratio))
//                 k (a = |x|; every k is 0 outside its support, which rounding can reach):
//                     box       1 for -0.5 <= x < 0.5
//                     tent      1 - a                                                         a < 1
//                     mitchell  (((21 * a - 36) * a) * a + 16) / 18                           a < 1       (B = C = 1/3, times 3)
//                               (((-7 * a + 36) * a - 60) * a + 32) / 18                     1 <= a < 2
//                     lanczos3  1 at x == 0;  0 at a >= 3 and at every other x == rint(x);  else with p = pi * x, q = p / 3:
//                               (sin(p) / p) * (sin(q) / q)
//   3. horizontal P(i, y) = sum over t = 0 .. T_x - 1 of wx_it * s(clamp(first_i + t, 0, w - 1), y), as acc = 0; acc = acc + w * v:
//                 the product is rounded, then the sum.  ALL T_x taps are taken, the padded ones too (their weight is 0).  A tap
//                 clamped to the border keeps its own weight: edge replication.  P is W x h.
//   4. vertical   the same over the rows of P with the y table -> W x H.
//   5. clamp      clamp_negative:  out = acc >= 0 ? acc : 0  (mitchell and lanczos3 have negative lobes).
//   6. alpha      out.a = the input's a at (nearest_x, nearest_y): not filtered, not divided by n.
// With W x H = w x h, tent and lanczos3 rows are one weight 1.0 and zeros, and 0 + 1 * v + 0 * u = v: the output is the sanitised
// mean bit for bit.  Every index is clamped before it is used: no address outside a plane is ever formed.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "bt_glare.hpp"

#define BT_RESAMPLE_HD BT_GLARE_HD
#define BT_RESAMPLE_MAX_TAPS 128
#define BT_RESAMPLE_FILTERS 4          // box, tent, mitchell, lanczos3 = 0 .. 3 (bt_resample_filter)

namespace btresample {

using btglare::Texel;

// ---- step 3 / 4: one tap, one output texel of one pass ----
BT_RESAMPLE_HD uint32_t clamp_index(int64_t p, uint32_t side) { return p < 0 ? 0u : p > (int64_t)side - 1 ? side - 1u : (uint32_t)p; }

template <class T>
BT_RESAMPLE_HD T tap(T acc, float w, T v) {
    acc.x = acc.x + w * v.x;
    acc.y = acc.y + w * v.y;
    acc.z = acc.z + w * v.z;
    acc.w = acc.w + w * v.w;
    return acc;
}
// `weights`: the row's `taps` weights; `first`: its first (unclamped) tap; `side`: the texels of the source axis
template <class T, class F>
BT_RESAMPLE_HD T filter_texel(F fetch, const float *weights, int32_t first, uint32_t taps, uint32_t side) {
    T acc;
    acc.x = acc.y = acc.z = acc.w = 0.0f;
    for (uint32_t t = 0; t < taps; ++t) acc = tap<T>(acc, weights[t], fetch(clamp_index((int64_t)first + t, side)));
    return acc;
}
// ---- steps 5 and 6 ----
BT_RESAMPLE_HD float finish1(float acc, int clamp_negative) { return clamp_negative ? (acc >= 0.0f ? acc : 0.0f) : acc; }
template <class T>
BT_RESAMPLE_HD T finish(T acc, int clamp_negative, float alpha) {
    T o;
    o.x = finish1(acc.x, clamp_negative);
    o.y = finish1(acc.y, clamp_negative);
    o.z = finish1(acc.z, clamp_negative);
    o.w = alpha;
    return o;
}

// ---- step 2 (host, float64) ----
inline double radius(int filter) { return filter == 0 ? 0.5 : filter == 1 ? 1.0 : filter == 2 ? 2.0 : 3.0; }
inline const char *filter_name(int filter) { return filter == 0 ? "box" : filter == 1 ? "tent" : filter == 2 ? "mitchell" : "lanczos3"; }

inline double kernel(int filter, double x) {
    const double a = x < 0.0 ? -x : x;
    switch (filter) {
    case 0: return x >= -0.5 && x < 0.5 ? 1.0 : 0.0;
    case 1: return a < 1.0 ? 1.0 - a : 0.0;
    case 2:
        if (a < 1.0) return (((21.0 * a - 36.0) * a) * a + 16.0) / 18.0;
        if (a < 2.0) return (((-7.0 * a + 36.0) * a - 60.0) * a + 32.0) / 18.0;
        return 0.0;
    default: {
        if (x == 0.0) return 1.0;
        if (a >= 3.0 || x == rint(x)) return 0.0;
        const double p = 3.14159265358979323846 * x, q = p / 3.0;
        return (sin(p) / p) * (sin(q) / q);
    }
    }
}

struct Span {
    double ratio, s, reach;              // reach = R * s
};
inline Span span_of(uint32_t src, uint32_t dst, int filter) {
    Span g;
    g.ratio = (double)src / (double)dst;
    g.s = g.ratio > 1.0 ? g.ratio : 1.0;
    g.reach = radius(filter) * g.s;
    return g;
}
inline void row_taps(const Span &g, uint32_t i, int64_t &first, int64_t &last, double &c) {
    c = ((double)i + 0.5) * g.ratio - 0.5;
    first = (int64_t)ceil(c - g.reach);
    last = (int64_t)floor(c + g.reach);
}
// T of an axis: the rows are walked until one has more than `limit` taps.
inline uint64_t max_taps(uint32_t src, uint32_t dst, int filter, uint64_t limit = ~0ull) {
    const Span g = span_of(src, dst, filter);
    uint64_t T = 1;
    for (uint32_t i = 0; i < dst && T <= limit; ++i) {
        int64_t first, last;
        double c;
        row_taps(g, i, first, last, c);
        const uint64_t n = last >= first ? (uint64_t)(last - first + 1) : 0;
        if (n > T) T = n;
    }
    return T;
}
// Whether T exceeds `limit`; `taps` receives T, or where it is far from the limit the 2 R s a row has about: the rows are then
// not walked (an axis may have 2^32 - 1 of them).
inline bool taps_exceed(uint32_t src, uint32_t dst, int filter, uint64_t limit, double &taps) {
    const double about = floor(2.0 * span_of(src, dst, filter).reach);
    taps = about;
    if (about - 2.0 > (double)limit) return true;
    if (about + 2.0 <= (double)limit) return false;
    taps = (double)max_taps(src, dst, filter, limit);
    return taps > (double)limit;
}

struct Axis {
    uint32_t src = 0, dst = 0, taps = 0;
    int filter = -1;
    std::vector<int32_t> first;          // [dst], unclamped
    std::vector<float> weights;          // [dst][taps]
    std::vector<uint32_t> nearest;       // [dst]
    bool is(uint32_t s, uint32_t d, int f) const { return filter == f && src == s && dst == d; }
    // the source texels that `n` consecutive outputs from `i0` take, all taps clamped: their first and their count
    uint32_t reach_of(uint32_t i0, uint32_t n, uint32_t &origin) const {
        const uint32_t i1 = i0 + n < dst ? i0 + n - 1 : dst - 1;
        origin = clamp_index(first[i0], src);
        return clamp_index((int64_t)first[i1] + taps - 1, src) - origin + 1;
    }
    // the largest of them over the tiles of `n` outputs
    uint32_t widest(uint32_t n) const {
        uint32_t m = 0, origin;
        for (uint64_t i0 = 0; i0 < dst; i0 += n) {
            const uint32_t r = reach_of((uint32_t)i0, n, origin);
            if (r > m) m = r;
        }
        return m;
    }
};

inline void build_axis(Axis &ax, uint32_t src, uint32_t dst, int filter) {
    const Span g = span_of(src, dst, filter);
    const uint32_t T = (uint32_t)max_taps(src, dst, filter, 0xffffffffull);
    ax.src = src;
    ax.dst = dst;
    ax.filter = filter;
    ax.taps = T;
    ax.first.assign(dst, 0);
    ax.nearest.assign(dst, 0);
    ax.weights.assign((size_t)dst * T, 0.0f);
    std::vector<double> k(T);
    for (uint32_t i = 0; i < dst; ++i) {
        int64_t first, last;
        double c;
        row_taps(g, i, first, last, c);
        double sum = 0.0;
        uint32_t n = 0;
        for (int64_t j = first; j <= last; ++j, ++n) {
            k[n] = kernel(filter, ((double)j - c) / g.s);
            sum = sum + k[n];
        }
        for (uint32_t t = 0; t < n; ++t) ax.weights[(size_t)i * T + t] = (float)(k[t] / sum);
        ax.first[i] = (int32_t)first;
        const double near = floor(((double)i + 0.5) * g.ratio);
        ax.nearest[i] = near < (double)(src - 1u) ? (uint32_t)near : src - 1u;
    }
}

// ---- the whole definition on the host: `plane` (W x h) and `out` (W x H) are blocks of exactly their size ----
inline void run_host(const Texel *rgba, uint32_t samples, uint32_t w, uint32_t h, Texel *out, uint32_t W, uint32_t H, const Axis &ax,
                     const Axis &ay, float max_value, int clamp_negative, Texel *plane) {
    const float r = 1.0f / (float)samples;
    for (uint32_t y = 0; y < h; ++y) {
        const Texel *row = rgba + (size_t)y * w;
        for (uint32_t i = 0; i < W; ++i)
            plane[(size_t)y * W + i] = filter_texel<Texel>([&](uint32_t p) { return btglare::sanitise(row[p], r, max_value); },
                                                          &ax.weights[(size_t)i * ax.taps], ax.first[i], ax.taps, w);
    }
    for (uint32_t j = 0; j < H; ++j)
        for (uint32_t i = 0; i < W; ++i) {
            const Texel acc = filter_texel<Texel>([&](uint32_t p) { return plane[(size_t)p * W + i]; }, &ay.weights[(size_t)j * ay.taps],
                                                  ay.first[j], ay.taps, h);
            out[(size_t)j * W + i] = finish(acc, clamp_negative, rgba[(size_t)ay.nearest[j] * w + ax.nearest[i]].w);
        }
}

} // namespace btresample

// The launchers of bt_resample.hip, for the two files of the library that define and call them (both include
// <hip/hip_runtime.h> and define BT_RESAMPLE_LAUNCHERS first).  hipErrorInvalidConfiguration for a plane whose tiles do not fit
// one launch.
#ifdef BT_RESAMPLE_LAUNCHERS
// Build knob (DESIGN.md 17 has both forms' times; they are bit-identical).  BT_RESAMPLE_LDS: the horizontal pass stages the source
// span of its 32 x 8 outputs in LDS where a row has BT_RESAMPLE_STAGE_MIN_TAPS taps and more and that span fits
// (BT_RESAMPLE_STAGE_X texels of a row), and takes the direct form (a clamped global load per tap) elsewhere; 0 builds the
// direct form alone.  The vertical pass is direct in both builds.
#ifndef BT_RESAMPLE_LDS
#define BT_RESAMPLE_LDS 1
#endif
#define BT_RESAMPLE_TILE_X 32
#define BT_RESAMPLE_TILE_Y 8
#define BT_RESAMPLE_STAGE_X 192        // 8 rows x 192 texels x 16 B = 24 KiB: six workgroups of four waves per CU
#define BT_RESAMPLE_STAGE_MIN_TAPS 6    // measured: staged wins at 6, 7 and 12 taps a row, direct at 2, 3 and 4
// One axis table on the device: first[dst], nearest[dst], weights[dst][taps].
struct BtResampleAxis {
    const int32_t *first;
    const uint32_t *nearest;
    const float *weights;
    uint32_t taps;
    uint32_t widest;                   // the widest source span of a tile of 32 outputs (Axis::widest); read for the x axis
};
extern "C" {
// sums (w x h running sums) -> plane (W x h)
hipError_t bt_launch_resample_h(const float *sums, uint32_t samples, float max_value, uint32_t w, uint32_t h, float *plane, uint32_t W,
                                BtResampleAxis ax, hipStream_t stream);
// plane (W x h) -> out (W x H); the alpha from sums at (ax.nearest, ay.nearest)
hipError_t bt_launch_resample_v(const float *plane, uint32_t W, uint32_t h, float *out, uint32_t H, BtResampleAxis ay,
                                const uint32_t *nearest_x, const float *sums, uint32_t w, int clamp_negative, hipStream_t stream);
}
#endif
