// bt_despeckle_api.cpp -- EXTENSION, NOT IN THE REFERENCE: the C ABI of the despeckle stage (include/bendy_hip.h, bt_despeckle;
// DESIGN.md 18).  Validation, the handle's two counters and the launch; the kernel is in bt_despeckle.hip, the definition in
// bt_despeckle.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/bendy_hip.h"
#include "bt_internal.hpp"
#define BT_DESPECKLE_LAUNCHERS
#include "bt_despeckle.hpp"

#pragma STDC FP_CONTRACT OFF

struct bt_despeckle {
    int device = -1;
    uint32_t *counters = nullptr;       // {flagged, sanitised} of the last call, on `device`
    // the last call
    bool called = false;
    uint32_t pixels = 0;
    hipStream_t last_stream = nullptr;

    void release() {
        if (counters) (void)hipFree(counters);
        counters = nullptr;
    }
    ~bt_despeckle() {
        if (device >= 0 && counters) {
            int c = -1;
            if (hipGetDevice(&c) == hipSuccess && c != device) (void)hipSetDevice(device);
            release();
            if (c >= 0 && c != device) (void)hipSetDevice(c);
        }
    }
    // the counters on the current device (a handle that held some on another device starts afresh)
    int ensure() {
        int dev = -1;
        BT_HIP(hipGetDevice(&dev));
        if (counters && device != dev) {
            (void)hipSetDevice(device);
            release();
            BT_HIP(hipSetDevice(dev));
        }
        device = dev;
        if (counters) return 0;
        BT_HIP(hipMalloc((void **)&counters, 2 * sizeof(uint32_t)));
        return 0;
    }
};

namespace {

int check_args(const void *handle, const float *in, uint32_t samples, const float *out, uint32_t width, uint32_t height,
               const bt_despeckle_params &p, bool with_handle) {
    // in the order the header gives
    if ((with_handle && !handle) || !in || !out) return fail(BT_ERR_INVALID_ARG, "null despeckle handle, input or output buffer");
    if (samples == 0) return fail(BT_ERR_INVALID_ARG, "frame with 0 samples");
    if (width == 0 || height == 0 || (uint64_t)width * height > 0xffffffffull)
        return fail(BT_ERR_INVALID_ARG, "zero-sized or too large a frame");
    if (in == out) return fail(BT_ERR_INVALID_ARG, "the output must not alias the input: every neighbour value is the input's");
    if (p.radius < 1 || p.radius > BT_DESPECKLE_MAX_RADIUS)
        return fail(BT_ERR_INVALID_ARG, "bt_despeckle_params.radius " + std::to_string(p.radius) + " is neither 1 nor 2");
    if (p.rank == 0 || p.rank > btdespeckle::max_rank(p.radius))
        return fail(BT_ERR_INVALID_ARG, "bt_despeckle_params.rank " + std::to_string(p.rank) + " is outside 1 .. " +
                                            std::to_string(btdespeckle::max_rank(p.radius)) + ", the window's neighbours");
    if (!std::isfinite(p.ratio) || !(p.ratio >= 1.0f)) return fail(BT_ERR_INVALID_ARG, "bt_despeckle_params.ratio must be finite and >= 1");
    if (!std::isfinite(p.floor) || !(p.floor >= 0.0f)) return fail(BT_ERR_INVALID_ARG, "bt_despeckle_params.floor must be finite and >= 0");
    if (!std::isfinite(p.max_value) || !(p.max_value > 0.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_despeckle_params.max_value must be finite and > 0");
    return 0;
}

} // namespace

extern "C" {

void bt_despeckle_params_default(bt_despeckle_params *out) {
    if (!out) return;
    // starting values (DESIGN.md 18 has the sweep around them); max_value is the glare and resample stages' cap
    out->radius = 1;
    out->rank = 2;
    out->ratio = 4.0f;
    out->floor = 0.01f;
    out->max_value = 65536.0f;
}

bt_despeckle *bt_despeckle_new(void) { return new bt_despeckle(); }

void bt_despeckle_free(bt_despeckle *h) { delete h; }

int bt_despeckle_device(bt_despeckle *h, const float *rgba_device, uint32_t samples, float *out_device, uint32_t width, uint32_t height,
                        const bt_despeckle_params *params, void *stream) {
    bt_despeckle_params p;
    if (params) p = *params;
    else bt_despeckle_params_default(&p);
    int rc = check_args(h, rgba_device, samples, out_device, width, height, p, true);
    if (rc) return rc;
    rc = h->ensure();
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    h->called = false;                   // until the launch below has been enqueued
    const float fn = (float)samples, cap = p.max_value * fn, fl = p.floor * fn;
    BT_HIP(hipMemsetAsync(h->counters, 0, 2 * sizeof(uint32_t), s));
    BT_HIP(bt_launch_despeckle(rgba_device, out_device, width, height, p.radius, p.rank, p.ratio, fl, cap, h->counters, s));
    h->pixels = (uint32_t)((uint64_t)width * height);
    h->last_stream = s;
    h->called = true;
    return 0;
}

int bt_despeckle_poll(bt_despeckle *h, bt_despeckle_stats *out) {
    if (!h || !out) return fail(BT_ERR_INVALID_ARG, "null despeckle handle or stats");
    if (!h->called || !h->counters) return fail(BT_ERR_INVALID_ARG, "bt_despeckle_poll before a bt_despeckle_device call");
    uint32_t c[2] = {0, 0};
    BT_HIP(hipStreamSynchronize(h->last_stream));
    BT_HIP(hipMemcpy(c, h->counters, sizeof c, hipMemcpyDeviceToHost));
    out->flagged = c[0];
    out->sanitised = c[1];
    out->pixels = h->pixels;
    out->reserved = 0;
    return 0;
}

int bt_debug_despeckle_host(const float *rgba_host, uint32_t samples, float *out_host, uint32_t width, uint32_t height,
                            const bt_despeckle_params *params, bt_despeckle_stats *stats) {
    bt_despeckle_params p;
    if (params) p = *params;
    else bt_despeckle_params_default(&p);
    int rc = check_args(nullptr, rgba_host, samples, out_host, width, height, p, false);
    if (rc) return rc;
    static_assert(sizeof(btdespeckle::Texel) == 16, "a texel is four floats");
    uint64_t flagged = 0, sanitised = 0;
    btdespeckle::run_host((const btdespeckle::Texel *)rgba_host, samples, (btdespeckle::Texel *)out_host, width, height, p.radius, p.rank,
                          p.ratio, p.floor, p.max_value, &flagged, &sanitised);
    if (stats) {
        stats->flagged = (uint32_t)flagged;
        stats->sanitised = (uint32_t)sanitised;
        stats->pixels = (uint32_t)((uint64_t)width * height);
        stats->reserved = 0;
    }
    return 0;
}

} // extern "C"
