// bt_glare.hpp -- EXTENSION, NOT IN THE REFERENCE: the glare stage's definition, texel by texel (include/bendy_hip.h, bt_glare;
// DESIGN.md 16).  Plain __host__ __device__ code without a HIP runtime call: the kernels (bt_glare.hip), the host entry point
// bt_debug_glare_host and tests/cpp/glare_check.cpp run the same lines, so the whole stage is tested on a machine without a
// GPU.  Builds with a plain C++ compiler too.  tests/glare_ref.py restates it in numpy.
//
// Everything is float32 in the order written (-ffp-contract=off, correctly rounded division).  A texel type T is any struct of
// four floats x, y, z, w (float4 on the device, btglare::Texel on the host); `fetch(x, y)` returns the texel of a plane.
//
//   1. sanitise   r = 1 / n;  c = rgb * r;  s = c >= 0 ? c : 0  (NaN, negatives -> 0);  s = s < max_value ? s : max_value
//                 (+inf, fireflies -> max_value);  s.w = 0: the planes carry no alpha.
//   2. levels     L = min(levels, bit_length(max(width, height) - 1)); level k has sides ceil(side_{k-1} / 2); D_0 = s.
//   3. down       separable, x then y.  Per axis, output i takes the taps a, b, c, d at 2i-1, 2i, 2i+1, 2i+2, each clamped to
//                 [0, side_{k-1} - 1]:  t = b + c;  D = (((a + d) + t) + (t + t)) * 0.125     -- the binomial [1 3 3 1] / 8
//   4. weights    on the host in float64: p_1 = 1, p_k = p_{k-1} * (double)spread, S their sum in order, w_k = (float)(p_k / S).
//   5. up         A_L = D_L * w_L;  A_k = D_k * w_k + up(A_{k+1}).  up is separable, x then y.  Per axis, output x takes
//                 near = x >> 1 and far = near - 1 (x even) or near + 1 (x odd), both clamped to the coarser side:
//                 ((far + near) + (near + near)) * 0.25                                      -- the tent [1 3] / 4
//   6. composite  G = up(A_1);  out.rgb = s + (G - s) * strength;  out.a = the input's a.  `out` is a mean.
//   7. L = 0      out.rgb = s.
// Both filters are exact on a constant (2v, 2v, 4v, 4v, 8v, v and 2v, 2v, 4v, v), and every index is clamped before it is used: no
// address outside a plane is ever formed.
#pragma once
#include <stdint.h>

#include <memory>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BT_GLARE_HD __host__ __device__ inline
#else
#define BT_GLARE_HD inline
#endif

#define BT_GLARE_MAX_LEVELS 16

namespace btglare {

struct Texel {
    float x, y, z, w;
};

BT_GLARE_HD uint32_t half_side(uint32_t side) { return side / 2u + (side & 1u); }        // ceil(side / 2) without overflow

// bit_length(max(width, height) - 1): the halvings until both sides are 1
BT_GLARE_HD uint32_t effective_levels(uint32_t levels, uint32_t width, uint32_t height) {
    uint32_t m = (width > height ? width : height) - 1u, bits = 0;
    while (m) {
        ++bits;
        m >>= 1;
    }
    return levels < bits ? levels : bits;
}

// ---- step 1 ----
BT_GLARE_HD float sanitise1(float sum, float r, float max_value) {
    const float c = sum * r;
    float s = c >= 0.0f ? c : 0.0f;
    s = s < max_value ? s : max_value;
    return s;
}
template <class T>
BT_GLARE_HD T sanitise(T sums, float r, float max_value) {
    T s;
    s.x = sanitise1(sums.x, r, max_value);
    s.y = sanitise1(sums.y, r, max_value);
    s.z = sanitise1(sums.z, r, max_value);
    s.w = 0.0f;
    return s;
}

// ---- step 3 ----
BT_GLARE_HD float down1(float a, float b, float c, float d) {
    const float t = b + c;
    return (((a + d) + t) + (t + t)) * 0.125f;
}
template <class T>
BT_GLARE_HD T down4(T a, T b, T c, T d) {
    T o;
    o.x = down1(a.x, b.x, c.x, d.x);
    o.y = down1(a.y, b.y, c.y, d.y);
    o.z = down1(a.z, b.z, c.z, d.z);
    o.w = down1(a.w, b.w, c.w, d.w);
    return o;
}
// tap t (0 .. 3) of output i on an axis of `side` texels: 2i - 1 + t, clamped
BT_GLARE_HD uint32_t down_tap(uint32_t i, int t, uint32_t side) {
    const int64_t p = 2 * (int64_t)i - 1 + t;
    return p < 0 ? 0u : p > (int64_t)side - 1 ? side - 1u : (uint32_t)p;
}
// D_k(i, j) from the plane D_{k-1} of sw x sh texels
template <class T, class F>
BT_GLARE_HD T down_texel(F fetch, uint32_t i, uint32_t j, uint32_t sw, uint32_t sh) {
    const uint32_t x0 = down_tap(i, 0, sw), x1 = down_tap(i, 1, sw), x2 = down_tap(i, 2, sw), x3 = down_tap(i, 3, sw);
    T row[4];
    for (int t = 0; t < 4; ++t) {
        const uint32_t y = down_tap(j, t, sh);
        row[t] = down4<T>(fetch(x0, y), fetch(x1, y), fetch(x2, y), fetch(x3, y));       // x first
    }
    return down4<T>(row[0], row[1], row[2], row[3]);                                      // then y
}

// ---- step 5 ----
BT_GLARE_HD float up1(float far, float near) { return ((far + near) + (near + near)) * 0.25f; }
template <class T>
BT_GLARE_HD T up2(T far, T near) {
    T o;
    o.x = up1(far.x, near.x);
    o.y = up1(far.y, near.y);
    o.z = up1(far.z, near.z);
    o.w = up1(far.w, near.w);
    return o;
}
// the far tap of output x on an axis whose coarser side is `cs` (the near tap is x >> 1, always inside)
BT_GLARE_HD uint32_t up_far(uint32_t x, uint32_t cs) {
    const uint32_t near = x >> 1;
    if (x & 1u) return near + 1u < cs ? near + 1u : cs - 1u;
    return near > 0u ? near - 1u : 0u;
}
// up(A_{k+1})(x, y), the coarser plane being cw x ch texels
template <class T, class F>
BT_GLARE_HD T up_texel(F fetch, uint32_t x, uint32_t y, uint32_t cw, uint32_t ch) {
    const uint32_t xn = x >> 1, xf = up_far(x, cw), yn = y >> 1, yf = up_far(y, ch);
    const T rf = up2<T>(fetch(xf, yf), fetch(xn, yf));                                    // x first
    const T rn = up2<T>(fetch(xf, yn), fetch(xn, yn));
    return up2<T>(rf, rn);                                                                // then y
}
template <class T>
BT_GLARE_HD T scale(T d, float w) {
    T o;
    o.x = d.x * w;
    o.y = d.y * w;
    o.z = d.z * w;
    o.w = d.w * w;
    return o;
}
// A_k = D_k * w_k + up(A_{k+1})
template <class T>
BT_GLARE_HD T accumulate(T d, float w, T up) {
    T o = scale<T>(d, w);
    o.x = o.x + up.x;
    o.y = o.y + up.y;
    o.z = o.z + up.z;
    o.w = o.w + up.w;
    return o;
}

// ---- step 6 ----
template <class T>
BT_GLARE_HD T composite(T s, T g, float strength, float alpha) {
    T o;
    o.x = s.x + (g.x - s.x) * strength;
    o.y = s.y + (g.y - s.y) * strength;
    o.z = s.z + (g.z - s.z) * strength;
    o.w = alpha;
    return o;
}

// ---- step 4 (host) ----
inline void level_weights(uint32_t L, float spread, float *w /* [L + 1], w[0] unused */) {
    double p[BT_GLARE_MAX_LEVELS + 1], sum = 0.0;
    for (uint32_t k = 1; k <= L; ++k) {
        p[k] = k == 1 ? 1.0 : p[k - 1] * (double)spread;
        sum = sum + p[k];
    }
    w[0] = 0.0f;
    for (uint32_t k = 1; k <= L; ++k) w[k] = (float)(p[k] / sum);
}

// ---- the whole definition on the host, every plane a heap block of exactly its size ----
// rgba, out: width * height texels.  planes (optional): A_1 .. A_L of the call, [k - 1] = level k.
inline void run_host(const Texel *rgba, uint32_t samples, Texel *out, uint32_t width, uint32_t height, uint32_t levels, float spread,
                     float strength, float max_value, std::vector<std::vector<Texel>> *planes = nullptr) {
    const float r = 1.0f / (float)samples;
    const uint32_t L = effective_levels(levels > BT_GLARE_MAX_LEVELS ? BT_GLARE_MAX_LEVELS : levels, width, height);
    if (planes) planes->clear();
    if (L == 0) {
        for (size_t i = 0; i < (size_t)width * height; ++i) {
            out[i] = sanitise(rgba[i], r, max_value);
            out[i].w = rgba[i].w;
        }
        return;
    }
    float w[BT_GLARE_MAX_LEVELS + 1];
    level_weights(L, spread, w);
    uint32_t pw[BT_GLARE_MAX_LEVELS + 1], ph[BT_GLARE_MAX_LEVELS + 1];
    pw[0] = width;
    ph[0] = height;
    std::unique_ptr<Texel[]> P[BT_GLARE_MAX_LEVELS + 1];
    for (uint32_t k = 1; k <= L; ++k) {
        pw[k] = half_side(pw[k - 1]);
        ph[k] = half_side(ph[k - 1]);
        P[k].reset(new Texel[(size_t)pw[k] * ph[k]]);
        Texel *dst = P[k].get();
        const Texel *src = P[k - 1].get();
        const uint32_t sw = pw[k - 1], sh = ph[k - 1];
        const float wl = k == L ? w[L] : 1.0f;                 // A_L = D_L * w_L; x * 1 is x
        for (uint32_t j = 0; j < ph[k]; ++j)
            for (uint32_t i = 0; i < pw[k]; ++i) {
                Texel d;
                if (k == 1)
                    d = down_texel<Texel>([&](uint32_t x, uint32_t y) { return sanitise(rgba[(size_t)y * sw + x], r, max_value); }, i, j, sw, sh);
                else
                    d = down_texel<Texel>([&](uint32_t x, uint32_t y) { return src[(size_t)y * sw + x]; }, i, j, sw, sh);
                dst[(size_t)j * pw[k] + i] = scale(d, wl);
            }
    }
    for (uint32_t k = L - 1; k >= 1; --k) {
        Texel *dst = P[k].get();
        const Texel *c = P[k + 1].get();
        const uint32_t cw = pw[k + 1], ch = ph[k + 1];
        for (uint32_t y = 0; y < ph[k]; ++y)
            for (uint32_t x = 0; x < pw[k]; ++x) {
                const Texel u = up_texel<Texel>([&](uint32_t a, uint32_t b) { return c[(size_t)b * cw + a]; }, x, y, cw, ch);
                Texel &d = dst[(size_t)y * pw[k] + x];
                d = accumulate(d, w[k], u);
            }
    }
    const Texel *a1 = P[1].get();
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const Texel in = rgba[(size_t)y * width + x];
            const Texel g = up_texel<Texel>([&](uint32_t a, uint32_t b) { return a1[(size_t)b * pw[1] + a]; }, x, y, pw[1], ph[1]);
            out[(size_t)y * width + x] = composite(sanitise(in, r, max_value), g, strength, in.w);
        }
    if (planes)
        for (uint32_t k = 1; k <= L; ++k) planes->emplace_back(P[k].get(), P[k].get() + (size_t)pw[k] * ph[k]);
}

} // namespace btglare

// The launchers of bt_glare.hip, for the two files of the library that define and call them (both include <hip/hip_runtime.h>
// and define BT_GLARE_LAUNCHERS first).  hipErrorInvalidConfiguration for a plane whose tiles do not fit one launch.
#ifdef BT_GLARE_LAUNCHERS
// Build knob (DESIGN.md 16 has both forms' times; they are bit-identical).  BT_GLARE_DOWN0_LDS: bt_glare_down0_kernel stages its
// 34 x 34 input texels in LDS; 0 builds the direct form.
#ifndef BT_GLARE_DOWN0_LDS
#define BT_GLARE_DOWN0_LDS 1
#endif
extern "C" {
hipError_t bt_launch_glare_down0(const float *sums, uint32_t samples, float max_value, uint32_t sw, uint32_t sh, float *dst,
                                 uint32_t dw, uint32_t dh, float w_out, hipStream_t stream);
hipError_t bt_launch_glare_down(const float *src, uint32_t sw, uint32_t sh, float *dst, uint32_t dw, uint32_t dh, float w_out,
                                hipStream_t stream);
hipError_t bt_launch_glare_up(float *plane, uint32_t w, uint32_t h, const float *coarse, uint32_t cw, uint32_t ch, float w_k,
                              hipStream_t stream);
hipError_t bt_launch_glare_composite(const float *sums, uint32_t samples, float max_value, float strength, const float *a1,
                                     uint32_t cw, uint32_t ch, float *out, uint32_t w, uint32_t h, hipStream_t stream);
hipError_t bt_launch_glare_mean(const float *sums, uint32_t samples, float max_value, float *out, uint64_t n, hipStream_t stream);
}
#endif
