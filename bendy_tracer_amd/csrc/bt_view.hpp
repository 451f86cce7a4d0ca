// bt_view.hpp -- EXTENSION, NOT IN THE REFERENCE: the camera as data (include/bendy_hip.h, bt_view) and its two maps, pixel ->
// world direction and world point -> pixel.  Plain __host__ __device__ code without a HIP runtime call: the
// temporal kernel (bt_temporal.hip), the host entry point bt_debug_reproject and tests/cpp/view_maps_check.cpp run the same
// lines, so the projection is tested on a machine without a GPU.  Builds with a plain C++ compiler too.
//
// The forward map restates Ray::with_frustum plus the camera transform (ray.rs:103-135, mod.rs:272-302) at the centre of the
// pixel's sample footprint: Subpixel(n) offsets the samples by i / n, each jittered by half a sub-pixel either way, so the
// footprint of pixel x is centred on x + (n - 1) / (2 n) -- on x itself without sub-sampling.  Depth-of-field origin jitter is
// ignored: the ray starts at the camera's translation.  float32 throughout; the trigonometry is the compiler's.
#pragma once
#include <cmath>
#include <math.h>
#include <stdint.h>

#include "../../include/bendy_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BT_VIEW_HD __host__ __device__ inline
#else
#define BT_VIEW_HD inline
#endif

namespace btview {

// A bt_view with what the maps need besides: the inverse of its linear part (computed on the host, once per call).
struct View {
    bt_view v;
    float inv[9];              // L^-1, columns as L's
    float pw, ph, cn;          // 2 (1 / width), 2 (1 / height) (buffer.rs:68-76) and the footprint's centre offset
};

// Host side.  false for a view the temporal stage refuses: a non-finite entry, a field of view <= 0, clip_max <= clip_min, a
// zero-sized frame or a linear part with |det| < 1e-12.
inline bool prepare(const bt_view &v, View &out) {
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(v.to_world[i])) return false;
    if (!std::isfinite(v.yfov) || !std::isfinite(v.xfov) || !(v.yfov > 0.0f) || !(v.xfov > 0.0f)) return false;
    if (!std::isfinite(v.clip_min) || !std::isfinite(v.clip_max) || !(v.clip_max > v.clip_min)) return false;
    if (v.width == 0 || v.height == 0) return false;
    const float *m = v.to_world;
    const double a = m[0], b = m[3], c = m[6], d = m[1], e = m[4], f = m[7], g = m[2], h = m[5], i = m[8];   // rows of L
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    if (!(std::fabs(det) >= 1e-12)) return false;
    out.v = v;
    // columns of the inverse = rows of the adjugate / det
    out.inv[0] = (float)((e * i - f * h) / det); out.inv[3] = (float)((c * h - b * i) / det); out.inv[6] = (float)((b * f - c * e) / det);
    out.inv[1] = (float)((f * g - d * i) / det); out.inv[4] = (float)((a * i - c * g) / det); out.inv[7] = (float)((c * d - a * f) / det);
    out.inv[2] = (float)((d * h - e * g) / det); out.inv[5] = (float)((b * g - a * h) / det); out.inv[8] = (float)((a * e - b * d) / det);
    out.pw = 2.0f * (1.0f / (float)v.width);
    out.ph = 2.0f * (1.0f / (float)v.height);
    const uint32_t n = v.subsample_n;
    out.cn = n <= 1 ? 0.0f : (float)(n - 1) / (float)(2 * n);
    return true;
}

// m (3 x 3, column-major) times p
BT_VIEW_HD void mul3(const float *m, const float *p, float *r) {
    r[0] = (m[0] * p[0] + m[3] * p[1]) + m[6] * p[2];
    r[1] = (m[1] * p[0] + m[4] * p[1]) + m[7] * p[2];
    r[2] = (m[2] * p[0] + m[5] * p[1]) + m[8] * p[2];
}

// Forward map: the world direction (unit length) of the ray through the footprint centre of pixel (x, y).
BT_VIEW_HD void forward(const View &V, float x, float y, float *d) {
    const float u = (x + V.cn) * V.pw - 1.0f, v = (y + V.cn) * V.ph - 1.0f;
    const float yrot = V.v.xfov * 0.5f * -u, xrot = V.v.yfov * 0.5f * -v;
    const float cx = cosf(xrot);
    const float local[3] = {-cx * sinf(yrot), sinf(xrot), -cx * cosf(yrot)};
    float w[3];
    mul3(V.v.to_world, local, w);
    const float l = sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    d[0] = w[0] / l; d[1] = w[1] / l; d[2] = w[2] / l;
}

// The camera focus that puts the point at distance t along forward(x, y) in the focal plane (bt_scene_pick): the render kernel
// aims a focused ray at origin + d * (focus / |d_cam.z|) (mod.rs:286-299) with d of unit length, so focus = t |d_cam.z|.
BT_VIEW_HD float focus_of(const View &V, float x, float y, float t) {
    const float u = (x + V.cn) * V.pw - 1.0f, v = (y + V.cn) * V.ph - 1.0f;                    // forward()'s lines: local[2] is d_cam.z
    const float yrot = V.v.xfov * 0.5f * -u, xrot = V.v.yfov * 0.5f * -v;
    return t * fabsf(-cosf(xrot) * cosf(yrot));
}

// Inverse map: the pixel coordinates at which the view sees the offset `p` from its origin (P - T for a point, a direction for a
// point at infinity).  Non-finite for p = 0.
BT_VIEW_HD void inverse(const View &V, const float *p, float *xf, float *yf) {
    float q[3];
    mul3(V.inv, p, q);
    const float l = sqrtf((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    const float ex = q[0] / l, ey = q[1] / l, ez = q[2] / l;
    const float xrot = asinf(fminf(fmaxf(ey, -1.0f), 1.0f)), yrot = atan2f(-ex, -ez);
    const float u = -yrot / (0.5f * V.v.xfov), v = -xrot / (0.5f * V.v.yfov);
    *xf = (u + 1.0f) / V.pw - V.cn;
    *yf = (v + 1.0f) / V.ph - V.cn;
}

// Where pixel (x, y) of `cur`, at normalised depth z (z >= 1: every sample missed, the point is at infinity), lies in `prev`:
// out = (x_f, y_f, z'), z' the point's normalised distance from prev's origin (1 at infinity).
BT_VIEW_HD void reproject(const View &cur, const View &prev, float x, float y, float z, float *out) {
    float d[3];
    forward(cur, x, y, d);
    if (z >= 1.0f) {
        inverse(prev, d, &out[0], &out[1]);
        out[2] = 1.0f;
        return;
    }
    const float t = cur.v.clip_min + z * (cur.v.clip_max - cur.v.clip_min);
    const float *T = cur.v.to_world + 9, *Tp = prev.v.to_world + 9;
    float p[3];
    for (int k = 0; k < 3; ++k) p[k] = (T[k] + t * d[k]) - Tp[k];
    const float r = sqrtf((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
    inverse(prev, p, &out[0], &out[1]);
    out[2] = (r - prev.v.clip_min) / (prev.v.clip_max - prev.v.clip_min);
}

} // namespace btview
