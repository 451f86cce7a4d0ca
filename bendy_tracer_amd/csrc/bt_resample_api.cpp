// bt_resample_api.cpp -- EXTENSION, NOT IN THE REFERENCE: the C ABI of the resample stage (include/bendy_hip.h, bt_resample;
// DESIGN.md 17).  Validation, the handle's tables and intermediate plane and the two launches; the kernels are in
// bt_resample.hip, the definition in bt_resample.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../include/bendy_hip.h"
#include "bt_internal.hpp"
#define BT_RESAMPLE_LAUNCHERS
#include "bt_resample.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

// one axis table's copy on the device: first[dst], nearest[dst], weights[dst][taps] in one allocation
struct DeviceAxis {
    char *mem = nullptr;
    size_t capacity = 0;                 // bytes
    uint32_t src = 0, dst = 0;           // what it holds (filter < 0: nothing)
    int filter = -1;
    bool is(const btresample::Axis &a) const { return filter == a.filter && src == a.src && dst == a.dst; }
};

} // namespace

struct bt_resample {
    int device = -1;
    btresample::Axis axis[2];            // x, y: the tables of the last call (device or host), kept for the next
    DeviceAxis dev[2];
    float *plane = nullptr;              // P: W x h float4
    size_t capacity = 0;                 // in texels
    // the last device call
    uint32_t pw = 0, ph = 0;
    bool have_plane = false;
    hipStream_t last_stream = nullptr;
    bool in_flight = false;              // a device call has been enqueued since the last synchronisation the handle knows of

    void release() {
        if (plane) (void)hipFree(plane);
        plane = nullptr;
        capacity = 0;
        for (DeviceAxis &d : dev) {
            if (d.mem) (void)hipFree(d.mem);
            d = DeviceAxis();
        }
        have_plane = false;
        in_flight = false;
    }
    ~bt_resample() {
        if (device >= 0 && (plane || dev[0].mem || dev[1].mem)) {
            int c = -1;
            if (hipGetDevice(&c) == hipSuccess && c != device) (void)hipSetDevice(device);
            release();
            if (c >= 0 && c != device) (void)hipSetDevice(c);
        }
    }
    // the handle on the current device (one that held memory on another device starts afresh)
    int bind() {
        int dev_now = -1;
        BT_HIP(hipGetDevice(&dev_now));
        if (device >= 0 && device != dev_now && (plane || dev[0].mem || dev[1].mem)) {
            (void)hipSetDevice(device);
            release();
            BT_HIP(hipSetDevice(dev_now));
        }
        device = dev_now;
        return 0;
    }
    // the host table of axis `a`; an upload of the table it replaces may still be reading it
    int table(int a, uint32_t src, uint32_t dst, int filter) {
        if (axis[a].is(src, dst, filter)) return 0;
        if (in_flight) {
            BT_HIP(hipStreamSynchronize(last_stream));
            in_flight = false;
        }
        btresample::build_axis(axis[a], src, dst, filter);
        return 0;
    }
    int upload(int a, hipStream_t s, BtResampleAxis &out) {
        const btresample::Axis &t = axis[a];
        DeviceAxis &d = dev[a];
        const size_t n_first = (size_t)t.dst * 4, n_w = (size_t)t.dst * t.taps * 4, bytes = 2 * n_first + n_w;
        if (!d.is(t)) {
            d.filter = -1;
            if (bytes > d.capacity) {
                if (d.mem) (void)hipFree(d.mem);     // hipFree waits for the work that still reads the old table
                d.mem = nullptr;
                d.capacity = 0;
                BT_HIP(hipMalloc((void **)&d.mem, bytes));
                d.capacity = bytes;
            }
            BT_HIP(hipMemcpyAsync(d.mem, t.first.data(), n_first, hipMemcpyHostToDevice, s));
            BT_HIP(hipMemcpyAsync(d.mem + n_first, t.nearest.data(), n_first, hipMemcpyHostToDevice, s));
            BT_HIP(hipMemcpyAsync(d.mem + 2 * n_first, t.weights.data(), n_w, hipMemcpyHostToDevice, s));
            d.src = t.src;
            d.dst = t.dst;
            d.filter = t.filter;
            last_stream = s;
            in_flight = true;
        }
        out.first = (const int32_t *)d.mem;
        out.nearest = (const uint32_t *)(d.mem + n_first);
        out.weights = (const float *)(d.mem + 2 * n_first);
        out.taps = t.taps;
        out.widest = a == 0 ? t.widest(BT_RESAMPLE_TILE_X) : 0;
        return 0;
    }
};

namespace {

bool bad_frame(uint32_t w, uint32_t h) {
    return w == 0 || h == 0 || (uint64_t)w * h > 0xffffffffull || w > 0x7fffffffu || h > 0x7fffffffu;
}

int check_args(const void *handle, const float *in, uint32_t samples, uint32_t w, uint32_t h, const float *out, uint32_t W, uint32_t H,
               const bt_resample_params &p, bool with_handle) {
    // in the order the header gives
    if ((with_handle && !handle) || !in || !out) return fail(BT_ERR_INVALID_ARG, "null resample handle, input or output buffer");
    if (samples == 0) return fail(BT_ERR_INVALID_ARG, "frame with 0 samples");
    if (bad_frame(w, h) || bad_frame(W, H)) return fail(BT_ERR_INVALID_ARG, "zero-sized or too large a frame (input or output)");
    if (in == out) return fail(BT_ERR_INVALID_ARG, "the output must not alias the input: the second pass re-reads the input's alpha");
    if (p.filter < 0 || p.filter >= BT_RESAMPLE_FILTERS)
        return fail(BT_ERR_INVALID_ARG, "bt_resample_params.filter " + std::to_string(p.filter) + " is not a bt_resample_filter");
    if (!std::isfinite(p.max_value) || !(p.max_value > 0.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_resample_params.max_value must be finite and > 0");
    const uint32_t src[2] = {w, h}, dst[2] = {W, H};
    for (int a = 0; a < 2; ++a) {
        double taps;
        if (btresample::taps_exceed(src[a], dst[a], p.filter, BT_RESAMPLE_MAX_TAPS, taps)) {
            char msg[256];
            std::snprintf(msg, sizeof msg, "the %c axis, %u -> %u (ratio %.4g : 1), takes about %.0f taps with %s: more than %d", a == 0 ? 'x' : 'y',
                          src[a], dst[a], (double)src[a] / (double)dst[a], taps, btresample::filter_name(p.filter), BT_RESAMPLE_MAX_TAPS);
            return fail(BT_ERR_INVALID_ARG, msg);
        }
    }
    return 0;
}

bt_resample_params params_or_default(const bt_resample_params *params) {
    bt_resample_params p;
    if (params) p = *params;
    else bt_resample_params_default(&p);
    return p;
}

} // namespace

extern "C" {

void bt_resample_params_default(bt_resample_params *out) {
    if (!out) return;
    out->filter = BT_RESAMPLE_MITCHELL;
    out->max_value = 65536.0f;           // the glare stage's cap, the display meter's `over` boundary
    out->clamp_negative = 1;
}

bt_resample *bt_resample_new(void) { return new bt_resample(); }

void bt_resample_free(bt_resample *h) { delete h; }

int bt_resample_device(bt_resample *h, const float *rgba_device, uint32_t samples, uint32_t width, uint32_t height, float *out_device,
                       uint32_t out_width, uint32_t out_height, const bt_resample_params *params, void *stream) {
    const bt_resample_params p = params_or_default(params);
    int rc = check_args(h, rgba_device, samples, width, height, out_device, out_width, out_height, p, true);
    if (rc) return rc;
    rc = h->bind();                      // BT_ERR_DEVICE without a device, before any table is built
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    h->have_plane = false;               // until both launches have been enqueued
    if ((rc = h->table(0, width, out_width, p.filter)) || (rc = h->table(1, height, out_height, p.filter))) return rc;
    const size_t texels = (size_t)out_width * height;
    if (texels > h->capacity) {
        if (h->plane) (void)hipFree(h->plane);       // hipFree waits for the work that still reads the old plane
        h->plane = nullptr;
        h->capacity = 0;
        BT_HIP(hipMalloc((void **)&h->plane, texels * 16));
        h->capacity = texels;
    }
    BtResampleAxis ax, ay;
    if ((rc = h->upload(0, s, ax)) || (rc = h->upload(1, s, ay))) return rc;
    h->last_stream = s;
    h->in_flight = true;
    BT_HIP(bt_launch_resample_h(rgba_device, samples, p.max_value, width, height, h->plane, out_width, ax, s));
    BT_HIP(bt_launch_resample_v(h->plane, out_width, height, out_device, out_height, ay, ax.nearest, rgba_device, width,
                                p.clamp_negative != 0, s));
    h->pw = out_width;
    h->ph = height;
    h->have_plane = true;
    return 0;
}

int bt_debug_resample_weights(bt_resample *h, int axis, uint32_t *sides, int32_t *first, float *weights, uint32_t *nearest) {
    if (!h) return fail(BT_ERR_INVALID_ARG, "null resample handle");
    if (axis != 0 && axis != 1) return fail(BT_ERR_INVALID_ARG, "axis " + std::to_string(axis) + ": 0 is x, 1 is y");
    const btresample::Axis &t = h->axis[axis];
    if (t.filter < 0) return fail(BT_ERR_INVALID_ARG, "the handle has no table yet: there has been no call");
    if (sides) {
        sides[0] = t.src;
        sides[1] = t.dst;
        sides[2] = (uint32_t)t.filter;
    }
    if (first) std::copy(t.first.begin(), t.first.end(), first);
    if (weights) std::copy(t.weights.begin(), t.weights.end(), weights);
    if (nearest) std::copy(t.nearest.begin(), t.nearest.end(), nearest);
    return (int)t.taps;
}

int bt_debug_resample_plane(bt_resample *h, float *host, uint32_t n) {
    if (!h) return fail(BT_ERR_INVALID_ARG, "null resample handle");
    if (!h->have_plane || !h->plane) return fail(BT_ERR_INVALID_ARG, "the handle has no plane: there has been no device call");
    const uint64_t count = (uint64_t)h->pw * h->ph * 4;
    if (count > 0x7fffffffull) return fail(BT_ERR_INVALID_ARG, "the plane has more elements than the return value can count");
    if (n == 0) return (int)count;
    if (!host) return fail(BT_ERR_INVALID_ARG, "null buffer");
    n = (uint32_t)std::min<uint64_t>(n, count);
    BT_HIP(hipStreamSynchronize(h->last_stream));
    h->in_flight = false;
    BT_HIP(hipMemcpy(host, h->plane, (size_t)n * 4, hipMemcpyDeviceToHost));
    return (int)n;
}

int bt_debug_resample_host(bt_resample *h, const float *rgba_host, uint32_t samples, uint32_t width, uint32_t height, float *out_host,
                           uint32_t out_width, uint32_t out_height, const bt_resample_params *params) {
    const bt_resample_params p = params_or_default(params);
    int rc = check_args(nullptr, rgba_host, samples, width, height, out_host, out_width, out_height, p, false);
    if (rc) return rc;
    static_assert(sizeof(btresample::Texel) == 16, "a texel is four floats");
    btresample::Axis local[2];
    btresample::Axis *ax = &local[0], *ay = &local[1];
    if (h) {                             // the handle keeps the tables, for bt_debug_resample_weights and for the next call
        if ((rc = h->table(0, width, out_width, p.filter)) || (rc = h->table(1, height, out_height, p.filter))) return rc;
        ax = &h->axis[0];
        ay = &h->axis[1];
    } else {
        btresample::build_axis(local[0], width, out_width, p.filter);
        btresample::build_axis(local[1], height, out_height, p.filter);
    }
    std::unique_ptr<btresample::Texel[]> plane(new btresample::Texel[(size_t)out_width * height]);
    btresample::run_host((const btresample::Texel *)rgba_host, samples, width, height, (btresample::Texel *)out_host, out_width, out_height,
                         *ax, *ay, p.max_value, p.clamp_negative != 0, plane.get());
    return 0;
}

} // extern "C"
