// bt_despeckle.hpp -- EXTENSION, NOT IN THE REFERENCE: the despeckle stage's definition, pixel by pixel (include/bendy_hip.h,
// bt_despeckle).  Plain __host__ __device__ code without a HIP runtime call: the kernel (bt_despeckle.hip), the host
// entry point bt_debug_despeckle_host and tests/cpp/despeckle_check.cpp run the same lines, so the whole stage is tested on a
// machine without a GPU.  Builds with a plain C++ compiler too.  tests/despeckle_ref.py restates it in numpy.
//
// Everything is float32 in the order written (-ffp-contract=off, correctly rounded division).  A texel type T is any struct of
// four floats x, y, z, w (float4 on the device, btdespeckle::Texel on the host).  The input is a frame of running sums of n
// samples, and so is the output: nothing is divided by n.
//
//   1. host       fn = (float)n;  cap = max_value * fn;  fl = floor * fn
//   2. sanitise   per channel of rgb:  s = v >= 0 ? v : 0  (NaN, negatives -> 0; -0.0 stays);  s = s < cap ? s : cap;
//                 Y = (0.2126 * s.x + 0.7152 * s.y) + 0.0722 * s.z                 -- the display meter's luminance
//   3. window     the in-frame pixels of the (2 radius + 1)^2 window, centre excluded; out-of-frame taps are absent, not clamped:
//                 M = (min(x + R, W - 1) - max(x - R, 0) + 1) * (min(y + R, H - 1) - max(y - R, 0) + 1) - 1;  k = min(rank, M)
//   4. select     T = the k-th largest neighbour Y (1 = the brightest).  An order statistic of non-negative finite floats: its
//                 value does not depend on how it is selected.  Absent taps are presented as -1, below every Y.
//   5. limit      lim = T * ratio + fl
//   6. apply      Y > lim (and M > 0): flagged, g = lim / Y, out.rgb = s * g;  else out.rgb = s.  out.a = the input's a.
// Every neighbour value is the input's: single pass, order-free.  No address outside the frame is ever formed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BT_DESPECKLE_HD __host__ __device__ inline
#else
#define BT_DESPECKLE_HD inline
#endif

#define BT_DESPECKLE_MAX_RADIUS 2
#define BT_DESPECKLE_MAX_TAPS 24                 // (2 * 2 + 1)^2 - 1

namespace btdespeckle {

struct Texel {
    float x, y, z, w;
};

BT_DESPECKLE_HD uint32_t max_rank(uint32_t radius) { return (2u * radius + 1u) * (2u * radius + 1u) - 1u; }

// ---- step 2 ----
BT_DESPECKLE_HD float sanitise1(float v, float cap) {
    float s = v >= 0.0f ? v : 0.0f;
    s = s < cap ? s : cap;
    return s;
}
// `changed`: step 2 replaced a channel (-0.0 and the cap itself pass unchanged)
template <class T>
BT_DESPECKLE_HD T sanitise(T v, float cap, bool &changed) {
    T s;
    s.x = sanitise1(v.x, cap);
    s.y = sanitise1(v.y, cap);
    s.z = sanitise1(v.z, cap);
    s.w = v.w;
    changed = !(s.x == v.x) || !(s.y == v.y) || !(s.z == v.z);
    return s;
}
template <class T>
BT_DESPECKLE_HD float luminance(T s) {
    return (0.2126f * s.x + 0.7152f * s.y) + 0.0722f * s.z;
}
// the luminance a neighbour presents to the selection
template <class T>
BT_DESPECKLE_HD float weigh(T v, float cap) {
    bool changed;
    return luminance(sanitise(v, cap, changed));
}

// ---- step 3 ----
BT_DESPECKLE_HD uint32_t span(uint32_t x, uint32_t radius, uint32_t side) {
    const uint32_t lo = x > radius ? x - radius : 0u;
    const uint32_t hi = side - 1u - x > radius ? x + radius : side - 1u;       // x + radius cannot wrap where it is taken
    return hi - lo + 1u;
}
BT_DESPECKLE_HD uint32_t neighbours(uint32_t x, uint32_t y, uint32_t radius, uint32_t width, uint32_t height) {
    return span(x, radius, width) * span(y, radius, height) - 1u;
}

// ---- step 4 ----
// Three forms of the same order statistic, none with an array that is indexed by a variable.  `tap(i)`, i = 0 .. N - 1, is the
// i-th neighbour's Y, or -1 for an absent one; 1 <= k <= M, the number of present ones.
// k <= 2: keep the two largest
template <int N, class F>
BT_DESPECKLE_HD float kth_top2(F tap, uint32_t k) {
    float a = -1.0f, b = -1.0f;                   // a >= b
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float v = tap(i);
        const float lo = v < a ? v : a;
        b = lo > b ? lo : b;
        a = v > a ? v : a;
    }
    return k == 1u ? a : b;
}
// k <= 4: keep the four largest; a value enters slot i where it is below slot i - 1
template <int N, class F>
BT_DESPECKLE_HD float kth_top4(F tap, uint32_t k) {
    float a = -1.0f, b = -1.0f, c = -1.0f, d = -1.0f;         // a >= b >= c >= d
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float v = tap(i);
        const float va = v < a ? v : a, vb = v < b ? v : b, vc = v < c ? v : c;
        d = vc > d ? vc : d;
        c = vb > c ? vb : c;
        b = va > b ? va : b;
        a = v > a ? v : a;
    }
    return k == 1u ? a : k == 2u ? b : k == 3u ? c : d;
}
// any k: the tap that fewer than k taps exceed and at least k taps reach.  Every tap with that property has the same value.
template <int N, class F>
BT_DESPECKLE_HD float kth_counting(F tap, uint32_t k) {
    float v[N];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = tap(i);
    float t = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        uint32_t above = 0, reach = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            above += v[j] > v[i] ? 1u : 0u;
            reach += v[j] >= v[i] ? 1u : 0u;
        }
        t = (above < k && k <= reach) ? v[i] : t;
    }
    return t;
}
template <int R, class F>
BT_DESPECKLE_HD float kth_largest(F tap, uint32_t rank, uint32_t k) {
    constexpr int N = (2 * R + 1) * (2 * R + 1) - 1;
    return rank <= 2u ? kth_top2<N>(tap, k) : rank <= 4u ? kth_top4<N>(tap, k) : kth_counting<N>(tap, k);
}
// the window offset of tap i (row-major, centre skipped)
template <int R>
BT_DESPECKLE_HD void tap_offset(int i, int &dx, int &dy) {
    constexpr int S = 2 * R + 1, C = (S * S) / 2;
    const int e = i < C ? i : i + 1;
    dx = e % S - R;
    dy = e / S - R;
}

// ---- steps 5 and 6 ----
BT_DESPECKLE_HD float limit(float T, float ratio, float fl) { return T * ratio + fl; }
template <class T>
BT_DESPECKLE_HD T apply(T s, float Y, float lim, uint32_t M, bool &flagged) {
    flagged = M > 0u && Y > lim;
    if (!flagged) return s;
    const float g = lim / Y;
    T o;
    o.x = s.x * g;
    o.y = s.y * g;
    o.z = s.z * g;
    o.w = s.w;
    return o;
}

// ---- the whole definition on the host, single-threaded; rgba and out are width * height texels ----
template <int R>
inline void run_host_radius(const Texel *rgba, Texel *out, uint32_t width, uint32_t height, uint32_t rank, float ratio, float fl, float cap,
                            uint64_t &n_flagged, uint64_t &n_sanitised) {
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            bool changed, flagged;
            const Texel s = sanitise(rgba[(size_t)y * width + x], cap, changed);
            const float Y = luminance(s);
            const uint32_t M = neighbours(x, y, (uint32_t)R, width, height), k = rank < M ? rank : M;
            float lim = 0.0f;
            if (M > 0u) {
                auto tap = [&](int i) {
                    int dx, dy;
                    tap_offset<R>(i, dx, dy);
                    const int64_t px = (int64_t)x + dx, py = (int64_t)y + dy;
                    if (px < 0 || py < 0 || px >= (int64_t)width || py >= (int64_t)height) return -1.0f;
                    return weigh(rgba[(size_t)py * width + (size_t)px], cap);
                };
                lim = limit(kth_largest<R>(tap, rank, k), ratio, fl);
            }
            out[(size_t)y * width + x] = apply(s, Y, lim, M, flagged);
            n_flagged += flagged ? 1u : 0u;
            n_sanitised += changed ? 1u : 0u;
        }
}
inline void run_host(const Texel *rgba, uint32_t samples, Texel *out, uint32_t width, uint32_t height, uint32_t radius, uint32_t rank,
                     float ratio, float floor, float max_value, uint64_t *n_flagged = nullptr, uint64_t *n_sanitised = nullptr) {
    const float fn = (float)samples, cap = max_value * fn, fl = floor * fn;
    uint64_t f = 0, s = 0;
    if (radius == 1u) run_host_radius<1>(rgba, out, width, height, rank, ratio, fl, cap, f, s);
    else run_host_radius<2>(rgba, out, width, height, rank, ratio, fl, cap, f, s);
    if (n_flagged) *n_flagged = f;
    if (n_sanitised) *n_sanitised = s;
}

} // namespace btdespeckle

// The launcher of bt_despeckle.hip, for the two files of the library that define and call it (both include <hip/hip_runtime.h>
// and define BT_DESPECKLE_LAUNCHERS first).  hipErrorInvalidConfiguration for a frame whose tiles do not fit one launch.
#ifdef BT_DESPECKLE_LAUNCHERS
// Build knob (DESIGN.md 18 has both forms' times; they are bit-identical).  BT_DESPECKLE_LDS: the kernel stages the luminances of
// its tile and halo in LDS; 0 builds the direct form, in which every thread fetches and weighs its own neighbours.
#ifndef BT_DESPECKLE_LDS
#define BT_DESPECKLE_LDS 1
#endif
extern "C" {
// counters: two uint32 on the device, {flagged, sanitised}, 8-byte aligned, zeroed by the caller on the same stream
hipError_t bt_launch_despeckle(const float *rgba, float *out, uint32_t width, uint32_t height, uint32_t radius, uint32_t rank,
                               float ratio, float fl, float cap, uint32_t *counters, hipStream_t stream);
}
#endif
