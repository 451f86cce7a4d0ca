// bt_upscale.hpp -- EXTENSION, NOT IN THE REFERENCE: the upscale stage's definition, pixel by pixel (include/bendy_hip.h,
// bt_upscale): joint bilateral upsampling of a small colour frame by the albedo, normal and depth guides of the
// shown size.  Plain __host__ __device__ code without a HIP runtime call: the kernels (bt_upscale.hip), the host entry point
// bt_debug_upscale_host and tests/cpp/upscale_check.cpp run the same lines, so the whole stage is tested on a machine without a
// GPU.  Builds with a plain C++ compiler too.  tests/upscale_ref.py restates it in numpy.
//
// Pixels are float32 in the order written (-ffp-contract=off); only + - * / and sqrt appear, all correctly rounded; there is no
// exp and no pow.  The per-axis tables are float64 on the host, rounded once to float32.  The input is a w x h frame of colour
// sums C with its count n_c and up to three guide PAIRS (albedo, normal, depth), each a w x h and a W x H frame of sums with
// their counts; the output is a W x H mean, W >= w and H >= h.  An absent pair weighs 1.
//
//   1. prepare    at either size, r = 1 / n once per frame:
//                     colour  c = btglare::sanitise(C.rgb, r): NaN and negatives -> 0, capped at max_value
//                     fin(v)  = |v| < inf ? v : 0  (a NaN fails the compare)
//                     albedo  a = fin(A.rgb * r_a)
//                     normal  v = fin(N.rgb * r_n);  l = (v.x v.x + v.y v.y) + v.z v.z;  n = l > 1e-12 ? v / sqrt(l) : 0.
//                             A zero normal (all three components == 0) marks a miss.
//                     depth   z = fin(Z.r * r_z)
//                 The lo planes are float4: (c.rgb, z), (n.xyz, 0), (a.rgb, 0).  An absent guide is all zeros at both sizes, which
//                 makes its weight exactly 1 (two misses; t = 0 / 1e-6; s = 0), and a product with 1 is exact.
//   2. tables     per axis (src -> dst texels), float64:  ratio = (double)src / dst;  c_i = (i + 0.5) * ratio - 0.5;
//                 x0 = floor(c_i);  f = c_i - x0;  the four taps are x0 - 1 + t, t = 0 .. 3, d_t = t - 1;  first_i = x0 - 1 is kept
//                 unclamped as int32 and a tap is clamped to [0, src - 1] where it is used, keeping its weight (edge replication);
//                     u1_t = (float)max(0, 1 - |d_t - f|)            the narrow (bilinear) weights
//                     u2_t = (float)max(0, 1 - |d_t - f| * 0.5)      the wide ones
//                     nearest_i = min(src - 1, floor((i + 0.5) * ratio))
//   3. per output pixel p, 16 taps q, ty outer and tx inner:
//                     g_n = 1 if both normals are zero, 0 if exactly one is, else m = max((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z, 0)
//                           and m = m * m, normal_squarings times
//                     g_z:  t = |z_p - z_q| / (sigma_depth * z_p + 1e-6);  g_z = 1 / (1 + t * t)
//                     g_a:  d = a_p - a_q;  s = (d.x d.x + d.y d.y) + d.z d.z;  g_a = 1 / (1 + s * k_a),  k_a = 1 / (sigma_albedo *
//                           sigma_albedo) in float32 on the host
//                     g = (g_n * g_z) * g_a;   s1 = u1y * u1x;  s2 = u2y * u2x;  w1 = s1 * g;  w2 = s2 * g
//                     A1 += w1 * c_q, D1 += w1;   A2 += w2 * c_q, D2 += w2;   A0 += s1 * c_q, D0 += s1
//                 each as acc = acc + w * c per channel, the product rounded, then the sum; all 16 taps, those of weight 0 too.
//   4. result     D1 > min_weight: A1 / D1 (tier 1);  else D2 > min_weight: A2 / D2 (tier 2);  else A0 / D0 (tier 3, plain
//                 bilinear).  A NaN weight fails both compares.  out.a = C.a at (nearest_x, nearest_y), neither filtered nor divided.
//   5. counters   the pixels that took tier 2 and tier 3.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "bt_glare.hpp"

#define BT_UPSCALE_HD BT_GLARE_HD
#define BT_UPSCALE_TILE 16
#define BT_UPSCALE_SPAN 19             // 16 outputs of an axis with dst >= src take at most 15 + 4 source texels

namespace btupscale {

using btglare::Texel;

struct Weights {                       // what the taps need of bt_upscale_params
    float sigma_depth, k_a, min_weight;
    uint32_t squarings;
};

// ---- step 1 ----
BT_UPSCALE_HD float fin(float v) { return (v < 0.0f ? -v : v) < __builtin_huge_valf() ? v : 0.0f; }
template <class T>
BT_UPSCALE_HD T prepare_albedo(T sums, float r) {
    T a;
    a.x = fin(sums.x * r);
    a.y = fin(sums.y * r);
    a.z = fin(sums.z * r);
    a.w = 0.0f;
    return a;
}
template <class T>
BT_UPSCALE_HD T prepare_normal(T sums, float r) {
    T v, n;
    v.x = fin(sums.x * r);
    v.y = fin(sums.y * r);
    v.z = fin(sums.z * r);
    const float l = (v.x * v.x + v.y * v.y) + v.z * v.z;
    n.x = n.y = n.z = n.w = 0.0f;
    if (l > 1e-12f) {
        const float s = sqrtf(l);
        n.x = v.x / s;
        n.y = v.y / s;
        n.z = v.z / s;
    }
    return n;
}
BT_UPSCALE_HD float prepare_depth(float sum, float r) { return fin(sum * r); }
// the first lo plane: (c.rgb, z)
template <class T>
BT_UPSCALE_HD T prepare_colour(T sums, float r, float max_value, float z) {
    T c = btglare::sanitise(sums, r, max_value);
    c.w = z;
    return c;
}
template <class T>
BT_UPSCALE_HD T zero_texel() {
    T t;
    t.x = t.y = t.z = t.w = 0.0f;
    return t;
}

// ---- step 3 ----
template <class T>
BT_UPSCALE_HD bool is_miss(T n) { return n.x == 0.0f && n.y == 0.0f && n.z == 0.0f; }

// the output pixel's own guides, and what of them every tap needs
template <class T>
struct Centre {
    T n, a;
    float z, z_den;
    bool miss;
};
template <class T>
BT_UPSCALE_HD Centre<T> centre_of(T n, T a, float z, const Weights &P) {
    Centre<T> p;
    p.n = n;
    p.a = a;
    p.z = z;
    p.z_den = P.sigma_depth * z + 1e-6f;
    p.miss = is_miss(n);
    return p;
}
// g of one tap: cz = (c.rgb, z), n, a of the lo texel
template <class T>
BT_UPSCALE_HD float guide_weight(const Centre<T> &p, T cz, T n, T a, const Weights &P) {
    float gn;
    const bool miss = is_miss(n);
    if (p.miss && miss) gn = 1.0f;
    else if (p.miss || miss) gn = 0.0f;
    else {
        const float d = (p.n.x * n.x + p.n.y * n.y) + p.n.z * n.z;
        gn = d > 0.0f ? d : 0.0f;
        for (uint32_t s = 0; s < P.squarings; ++s) gn = gn * gn;
    }
    const float dz = p.z - cz.w;
    const float t = (dz < 0.0f ? -dz : dz) / p.z_den;
    const float gz = 1.0f / (1.0f + t * t);
    const float dx = p.a.x - a.x, dy = p.a.y - a.y, dw = p.a.z - a.z;
    const float s = (dx * dx + dy * dy) + dw * dw;
    const float ga = 1.0f / (1.0f + s * P.k_a);
    return (gn * gz) * ga;
}

struct Sums {                          // A1 D1, A2 D2, A0 D0: the w of each texel is its D
    Texel one, two, zero;
};
template <class T>
BT_UPSCALE_HD void add(Texel &acc, float w, T c) {
    acc.x = acc.x + w * c.x;
    acc.y = acc.y + w * c.y;
    acc.z = acc.z + w * c.z;
    acc.w = acc.w + w;
}
template <class T>
BT_UPSCALE_HD void tap(Sums &S, const Centre<T> &p, T cz, T n, T a, float u1y, float u1x, float u2y, float u2x, const Weights &P) {
    const float g = guide_weight(p, cz, n, a, P);
    const float s1 = u1y * u1x, s2 = u2y * u2x;
    const float w1 = s1 * g, w2 = s2 * g;
    add(S.one, w1, cz);
    add(S.two, w2, cz);
    add(S.zero, s1, cz);
}
// ---- step 4: the tier is 1, 2 or 3 ----
template <class T>
BT_UPSCALE_HD T result(const Sums &S, float min_weight, float alpha, int &tier) {
    tier = S.one.w > min_weight ? 1 : S.two.w > min_weight ? 2 : 3;
    // selected among values, not among lvalues: a conditional between members is a choice of address and forces them into memory
    const Texel one = S.one, two = S.two, zero = S.zero;
    const bool t1 = tier == 1, t2 = tier == 2;
    const float lx = t2 ? two.x : zero.x, ly = t2 ? two.y : zero.y, lz = t2 ? two.z : zero.z, ld = t2 ? two.w : zero.w;
    const float ax = t1 ? one.x : lx, ay = t1 ? one.y : ly, az = t1 ? one.z : lz, d = t1 ? one.w : ld;
    T o;
    o.x = ax / d;
    o.y = ay / d;
    o.z = az / d;
    o.w = alpha;
    return o;
}
// One output pixel.  `fetch(tx, ty, cz, n, a)` hands out the three lo texels of tap (tx, ty), the clamp applied; ux / uy: the
// pixel's eight weights of each axis, narrow then wide.  Fully unrolled: no array is indexed by a variable.
template <class T, class F>
BT_UPSCALE_HD T pixel(F fetch, const Centre<T> &p, const float *ux, const float *uy, const Weights &P, float alpha, int &tier) {
    Sums S;
    S.one = S.two = S.zero = zero_texel<Texel>();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int ty = 0; ty < 4; ++ty) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int tx = 0; tx < 4; ++tx) {
            T cz, n, a;
            fetch(tx, ty, cz, n, a);
            tap<T>(S, p, cz, n, a, uy[ty], ux[tx], uy[4 + ty], ux[4 + tx], P);
        }
    }
    return result<T>(S, P.min_weight, alpha, tier);
}

BT_UPSCALE_HD uint32_t clamp_index(int64_t p, uint32_t side) { return p < 0 ? 0u : p > (int64_t)side - 1 ? side - 1u : (uint32_t)p; }

// ---- step 2 (host, float64) ----
struct Axis {
    uint32_t src = 0, dst = 0;
    std::vector<int32_t> first;          // [dst], unclamped: x0 - 1
    std::vector<float> weights;          // [dst][8]: u1_0 .. u1_3, u2_0 .. u2_3
    std::vector<uint32_t> nearest;       // [dst]
    bool is(uint32_t s, uint32_t d) const { return dst != 0 && src == s && dst == d; }
};

inline void build_axis(Axis &ax, uint32_t src, uint32_t dst) {
    const double ratio = (double)src / (double)dst;
    ax.src = src;
    ax.dst = dst;
    ax.first.assign(dst, 0);
    ax.nearest.assign(dst, 0);
    ax.weights.assign((size_t)dst * 8, 0.0f);
    for (uint32_t i = 0; i < dst; ++i) {
        const double c = ((double)i + 0.5) * ratio - 0.5, x0 = floor(c), f = c - x0;
        ax.first[i] = (int32_t)((int64_t)x0 - 1);
        for (int t = 0; t < 4; ++t) {
            const double d = fabs((double)(t - 1) - f), u1 = 1.0 - d, u2 = 1.0 - d * 0.5;
            ax.weights[(size_t)i * 8 + t] = (float)(u1 > 0.0 ? u1 : 0.0);
            ax.weights[(size_t)i * 8 + 4 + t] = (float)(u2 > 0.0 ? u2 : 0.0);
        }
        const double near = floor(((double)i + 0.5) * ratio);
        ax.nearest[i] = near < (double)(src - 1u) ? (uint32_t)near : src - 1u;
    }
}

// One frame's guides as the ABI hands them over: sums and counts, a NULL pointer for an absent guide.
struct Guides {
    const Texel *albedo, *normal, *depth;
    float r_albedo, r_normal, r_depth;   // 1 / count; anything where the pointer is NULL
};

// the three prepared texels of pixel `i` of a frame: colour (NULL at the shown size) and guides
inline void prepare(const Texel *colour, float r, float max_value, const Guides &g, size_t i, Texel &cz, Texel &n, Texel &a) {
    const float z = g.depth ? prepare_depth(g.depth[i].x, g.r_depth) : 0.0f;
    cz = colour ? prepare_colour(colour[i], r, max_value, z) : zero_texel<Texel>();
    cz.w = z;
    n = g.normal ? prepare_normal(g.normal[i], g.r_normal) : zero_texel<Texel>();
    a = g.albedo ? prepare_albedo(g.albedo[i], g.r_albedo) : zero_texel<Texel>();
}

// ---- the whole definition on the host: `planes` (3 planes of w x h) and `out` (W x H) are blocks of exactly their size ----
inline void run_host(const Texel *colour, uint32_t samples, uint32_t w, uint32_t h, const Guides &lo, const Guides &hi, Texel *out, uint32_t W,
                     uint32_t H, const Axis &ax, const Axis &ay, const Weights &P, float max_value, Texel *planes, uint64_t *tier2,
                     uint64_t *tier3) {
    const float r = 1.0f / (float)samples;
    const size_t texels = (size_t)w * h;
    Texel *pcz = planes, *pn = planes + texels, *pa = planes + 2 * texels;
    for (size_t i = 0; i < texels; ++i) prepare(colour, r, max_value, lo, i, pcz[i], pn[i], pa[i]);
    uint64_t n2 = 0, n3 = 0;
    for (uint32_t j = 0; j < H; ++j)
        for (uint32_t i = 0; i < W; ++i) {
            Texel cz, n, a;
            prepare(nullptr, 0.0f, 0.0f, hi, (size_t)j * W + i, cz, n, a);
            const Centre<Texel> p = centre_of(n, a, cz.w, P);
            const int32_t fx = ax.first[i], fy = ay.first[j];
            int tier = 0;
            out[(size_t)j * W + i] = pixel<Texel>(
                [&](int tx, int ty, Texel &qcz, Texel &qn, Texel &qa) {
                    const size_t q = (size_t)clamp_index((int64_t)fy + ty, h) * w + clamp_index((int64_t)fx + tx, w);
                    qcz = pcz[q];
                    qn = pn[q];
                    qa = pa[q];
                },
                p, &ax.weights[(size_t)i * 8], &ay.weights[(size_t)j * 8], P, colour[(size_t)ay.nearest[j] * w + ax.nearest[i]].w, tier);
            n2 += tier == 2;
            n3 += tier == 3;
        }
    if (tier2) *tier2 = n2;
    if (tier3) *tier3 = n3;
}

} // namespace btupscale

// The launchers of bt_upscale.hip, for the two files of the library that define and call them (both include
// <hip/hip_runtime.h> and define BT_UPSCALE_LAUNCHERS first).  hipErrorInvalidConfiguration for a frame whose tiles do not fit
// one launch.
#ifdef BT_UPSCALE_LAUNCHERS
// Build knob (DESIGN.md 19 has both forms' times; they are bit-identical).  BT_UPSCALE_LDS: the workgroup stages the 19 x 19
// footprint of the three lo planes in LDS and every tap is an LDS read; 0 builds the direct form, a clamped global load per tap.
#ifndef BT_UPSCALE_LDS
#define BT_UPSCALE_LDS 1
#endif
// One axis table on the device: first[dst], nearest[dst], weights[dst][8].
struct BtUpscaleAxis {
    const int32_t *first;
    const uint32_t *nearest;
    const float *weights;
};
// One frame's guide sums on the device; NULL for an absent guide.
struct BtUpscaleGuides {
    const float *albedo, *normal, *depth;
    float r_albedo, r_normal, r_depth;
};
extern "C" {
// colour sums and lo guides (w x h) -> the three prepared planes, `planes` holding 3 * w * h float4
hipError_t bt_launch_upscale_prepare(const float *colour, float r, float max_value, BtUpscaleGuides lo, uint32_t w, uint32_t h, float *planes,
                                     hipStream_t stream);
// planes and hi guides -> out (W x H); the alpha from `colour` at (ax.nearest, ay.nearest); counters: one uint64, zeroed by the caller
hipError_t bt_launch_upscale(const float *planes, const float *colour, uint32_t w, uint32_t h, BtUpscaleGuides hi, float *out, uint32_t W,
                             uint32_t H, BtUpscaleAxis ax, BtUpscaleAxis ay, btupscale::Weights P, unsigned long long *counters,
                             hipStream_t stream);
}
#endif
