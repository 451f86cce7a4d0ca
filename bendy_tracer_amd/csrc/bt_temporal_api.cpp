// bt_temporal_api.cpp -- EXTENSION, NOT IN THE REFERENCE: the C ABI of temporal accumulation with reprojection
// (include/bendy_hip.h, bt_temporal).  Validation, the handle's planes and the host side of the projection; the
// kernel is in bt_temporal.hip, the two maps in bt_view.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/bendy_hip.h"
#include "bt_internal.hpp"

#pragma STDC FP_CONTRACT OFF

struct bt_temporal {
    uint32_t width = 0, height = 0;
    int device = -1;
    // one allocation: history 0 | history 1 | guides 0 | guides 1, `pixels` float4 each (64 B per pixel)
    float *planes = nullptr;
    int cur = 0;                   // which of each pair the last accumulate wrote
    bool has_history = false;
    bt_view prev{};                // the view of the last accumulate (has_history)
    hipStream_t last_stream = nullptr;

    size_t pixels() const { return (size_t)width * height; }
    float4 *hist(int i) const { return (float4 *)planes + (size_t)i * pixels(); }
    float4 *guide(int i) const { return (float4 *)planes + (size_t)(2 + i) * pixels(); }
    void release() {
        if (planes) (void)hipFree(planes);
        planes = nullptr;
    }
    ~bt_temporal() {
        if (device >= 0 && planes) {
            int c = -1;
            if (hipGetDevice(&c) == hipSuccess && c != device) (void)hipSetDevice(device);
            release();
            if (c >= 0 && c != device) (void)hipSetDevice(c);
        }
    }
    // Planes on the current device (a handle that held some on another device starts afresh: their contents are gone).
    int ensure() {
        int dev = -1;
        BT_HIP(hipGetDevice(&dev));
        if (planes && device != dev) {
            (void)hipSetDevice(device);
            release();
            BT_HIP(hipSetDevice(dev));
            has_history = false;
        }
        device = dev;
        if (planes) return 0;
        BT_HIP(hipMalloc((void **)&planes, pixels() * 64));
        has_history = false;
        return 0;
    }
};

namespace {

int check_params(const bt_temporal_params &p) {
    if (!(p.alpha_min >= 0.0f && p.alpha_min <= 1.0f)) return fail(BT_ERR_INVALID_ARG, "bt_temporal_params.alpha_min must be in [0, 1]");
    if (!std::isfinite(p.max_history) || !(p.max_history >= 1.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_temporal_params.max_history must be finite and >= 1");
    if (!std::isfinite(p.depth_tolerance) || !(p.depth_tolerance >= 0.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_temporal_params.depth_tolerance must be finite and >= 0");
    if (!(p.normal_min >= -1.0f && p.normal_min <= 1.0f)) return fail(BT_ERR_INVALID_ARG, "bt_temporal_params.normal_min must be in [-1, 1]");
    return 0;
}

} // namespace

extern "C" {

void bt_temporal_params_default(bt_temporal_params *out) {
    if (!out) return;
    // chosen on scene / cornell2 at 128x128, eight frames of 1 x Subpixel(2) samples under a moving camera
    out->alpha_min = 0.05f;
    out->max_history = 256.0f;
    out->depth_tolerance = 0.05f;
    out->normal_min = 0.5f;
}

bt_temporal *bt_temporal_new(uint32_t width, uint32_t height) {
    if (width == 0 || height == 0 || (uint64_t)width * height > 0x7fffffffu) {
        fail(BT_ERR_INVALID_ARG, "bt_temporal_new: zero-sized or too large a frame");
        return nullptr;
    }
    bt_temporal *t = new bt_temporal();
    t->width = width;
    t->height = height;
    return t;
}

void bt_temporal_free(bt_temporal *t) { delete t; }

int bt_temporal_reset(bt_temporal *t) {
    if (!t) return fail(BT_ERR_INVALID_ARG, "null temporal handle");
    t->has_history = false;        // the next accumulate reads neither plane
    return 0;
}

int bt_temporal_accumulate_device(bt_temporal *t, const bt_view *view, const float *color, uint32_t color_samples,
                                  const float *normal, uint32_t normal_samples, const float *depth, uint32_t depth_samples,
                                  float *out, const bt_temporal_params *params, void *stream) {
    // everything that can be refused is refused before the device is touched, in the order the header gives
    if (!t || !view || !color || !depth || !out) return fail(BT_ERR_INVALID_ARG, "null handle, view, colour, depth or output buffer");
    if (color_samples == 0) return fail(BT_ERR_INVALID_ARG, "colour buffer with 0 samples");
    if (normal && normal_samples == 0) return fail(BT_ERR_INVALID_ARG, "normal buffer with 0 samples");
    if (depth_samples == 0) return fail(BT_ERR_INVALID_ARG, "depth buffer with 0 samples");
    if (view->width != t->width || view->height != t->height)
        return fail(BT_ERR_INVALID_ARG, "view of " + std::to_string(view->width) + "x" + std::to_string(view->height) +
                                            " on a temporal handle of " + std::to_string(t->width) + "x" + std::to_string(t->height));
    BtTemporalLaunch P{};
    if (!btview::prepare(*view, P.cur))
        return fail(BT_ERR_INVALID_ARG, "bt_view needs finite entries, yfov and xfov > 0, clip_max > clip_min and an invertible to_world");
    bt_temporal_params p;
    if (params) p = *params;
    else bt_temporal_params_default(&p);
    int rc = check_params(p);
    if (rc) return rc;
    if (out == color || out == normal || out == depth)
        return fail(BT_ERR_INVALID_ARG, "out must not alias an input: the inputs are running sums, out is a mean");

    rc = t->ensure();
    if (rc) return rc;
    int mode = 0;
    if (t->has_history) {
        mode = std::memcmp(&t->prev, view, sizeof(bt_view)) == 0 ? 1 : 2;
        if (!btview::prepare(t->prev, P.prev)) return fail(BT_ERR_INVALID_ARG, "the handle's previous view is invalid");   // (it was accepted)
    } else {
        P.prev = P.cur;
    }
    const int next = t->cur ^ 1;
    P.color = (const float4 *)color;
    P.normal = (const float4 *)normal;
    P.depth = (const float4 *)depth;
    P.nc = (float)color_samples;
    P.nn = (float)normal_samples;
    P.nd = (float)depth_samples;
    P.hist_in = t->hist(t->cur);
    P.guide_in = t->guide(t->cur);
    P.hist_out = t->hist(next);
    P.guide_out = t->guide(next);
    P.out = (float4 *)out;
    P.alpha_min = p.alpha_min;
    P.max_history = p.max_history;
    P.depth_tolerance = p.depth_tolerance;
    P.normal_min = p.normal_min;
    BT_HIP(bt_launch_temporal(&P, mode, (hipStream_t)stream));
    t->cur = next;
    t->has_history = true;
    t->prev = *view;
    t->last_stream = (hipStream_t)stream;
    return 0;
}

int bt_debug_temporal_history(bt_temporal *t, float *host, uint32_t n) {
    if (!t) return fail(BT_ERR_INVALID_ARG, "null temporal handle");
    const size_t total = t->pixels() * 4;
    if (n == 0) return (int)std::min<size_t>(total, 0x7fffffffu);
    if (!host) return fail(BT_ERR_INVALID_ARG, "null buffer");
    n = (uint32_t)std::min<size_t>(n, total);
    if (!t->has_history || !t->planes) {
        std::fill(host, host + n, 0.0f);
        return (int)n;
    }
    BT_HIP(hipStreamSynchronize(t->last_stream));
    BT_HIP(hipMemcpy(host, t->hist(t->cur), (size_t)n * 4, hipMemcpyDeviceToHost));
    return (int)n;
}

int bt_debug_reproject(const bt_view *cur, const bt_view *prev, float x, float y, float z, float *out) {
    if (!cur || !prev || !out) return fail(BT_ERR_INVALID_ARG, "null argument");
    btview::View c, p;
    if (!btview::prepare(*cur, c) || !btview::prepare(*prev, p))
        return fail(BT_ERR_INVALID_ARG, "bt_view needs finite entries, yfov and xfov > 0, clip_max > clip_min and an invertible to_world");
    btview::reproject(c, p, x, y, z, out);
    return 0;
}

} // extern "C"
