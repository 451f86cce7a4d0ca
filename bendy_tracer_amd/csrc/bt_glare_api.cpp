// bt_glare_api.cpp -- EXTENSION, NOT IN THE REFERENCE: the C ABI of the glare stage (include/bendy_hip.h, bt_glare;
// DESIGN.md 16).  Validation, the handle's pyramid and the sequence of launches; the kernels are in bt_glare.hip, the
// definition in bt_glare.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/bendy_hip.h"
#include "bt_internal.hpp"
#define BT_GLARE_LAUNCHERS
#include "bt_glare.hpp"

#pragma STDC FP_CONTRACT OFF

struct bt_glare {
    int device = -1;
    float *planes = nullptr;            // one allocation: the float4 planes of levels 1 .. L, one after the other
    size_t capacity = 0;                // in texels
    // the last call
    uint32_t L = 0;
    uint32_t pw[BT_GLARE_MAX_LEVELS + 1] = {}, ph[BT_GLARE_MAX_LEVELS + 1] = {};
    size_t at[BT_GLARE_MAX_LEVELS + 1] = {};     // a level's first texel
    hipStream_t last_stream = nullptr;

    float *plane(uint32_t k) const { return planes + 4 * at[k]; }
    void release() {
        if (planes) (void)hipFree(planes);
        planes = nullptr;
        capacity = 0;
    }
    ~bt_glare() {
        if (device >= 0 && planes) {
            int c = -1;
            if (hipGetDevice(&c) == hipSuccess && c != device) (void)hipSetDevice(device);
            release();
            if (c >= 0 && c != device) (void)hipSetDevice(c);
        }
    }
    // `texels` of planes on the current device (a handle that held some on another device starts afresh)
    int ensure(size_t texels) {
        int dev = -1;
        BT_HIP(hipGetDevice(&dev));
        if (planes && device != dev) {
            (void)hipSetDevice(device);
            release();
            BT_HIP(hipSetDevice(dev));
        }
        device = dev;
        if (texels <= capacity) return 0;
        release();                      // hipFree waits for the work that still reads the old planes
        L = 0;
        BT_HIP(hipMalloc((void **)&planes, texels * 16));
        capacity = texels;
        return 0;
    }
};

namespace {

int check_args(const void *handle, const float *in, uint32_t samples, const float *out, uint32_t width, uint32_t height,
               const bt_glare_params &p, bool with_handle) {
    // in the order the header gives
    if ((with_handle && !handle) || !in || !out) return fail(BT_ERR_INVALID_ARG, "null glare handle, input or output buffer");
    if (samples == 0) return fail(BT_ERR_INVALID_ARG, "frame with 0 samples");
    if (width == 0 || height == 0 || (uint64_t)width * height > 0xffffffffull)
        return fail(BT_ERR_INVALID_ARG, "zero-sized or too large a frame");
    if (in == out) return fail(BT_ERR_INVALID_ARG, "the output must not alias the input: the composite re-reads the sums");
    if (p.levels > BT_GLARE_MAX_LEVELS)
        return fail(BT_ERR_INVALID_ARG, "bt_glare_params.levels " + std::to_string(p.levels) + " exceeds 16");
    if (!std::isfinite(p.spread) || !(p.spread > 0.0f && p.spread <= 16.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_glare_params.spread must be finite and in (0, 16]");
    if (!(p.strength >= 0.0f && p.strength <= 1.0f)) return fail(BT_ERR_INVALID_ARG, "bt_glare_params.strength must be in [0, 1]");
    if (!std::isfinite(p.max_value) || !(p.max_value > 0.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_glare_params.max_value must be finite and > 0");
    return 0;
}

} // namespace

extern "C" {

void bt_glare_params_default(bt_glare_params *out) {
    if (!out) return;
    // starting values, not tuned; max_value is the display meter's `over` boundary
    out->levels = 6;
    out->spread = 1.0f;
    out->strength = 0.08f;
    out->max_value = 65536.0f;
}

bt_glare *bt_glare_new(void) { return new bt_glare(); }

void bt_glare_free(bt_glare *g) { delete g; }

int bt_glare_device(bt_glare *g, const float *rgba_device, uint32_t samples, float *out_device, uint32_t width, uint32_t height,
                    const bt_glare_params *params, void *stream) {
    bt_glare_params p;
    if (params) p = *params;
    else bt_glare_params_default(&p);
    int rc = check_args(g, rgba_device, samples, out_device, width, height, p, true);
    if (rc) return rc;

    const uint32_t L = btglare::effective_levels(p.levels, width, height);
    uint32_t pw[BT_GLARE_MAX_LEVELS + 1], ph[BT_GLARE_MAX_LEVELS + 1];
    size_t at[BT_GLARE_MAX_LEVELS + 1], texels = 0;
    pw[0] = width;
    ph[0] = height;
    at[0] = 0;
    for (uint32_t k = 1; k <= L; ++k) {
        pw[k] = btglare::half_side(pw[k - 1]);
        ph[k] = btglare::half_side(ph[k - 1]);
        at[k] = texels;
        texels += (size_t)pw[k] * ph[k];
    }
    rc = g->ensure(std::max<size_t>(texels, 1));
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    g->L = 0;                            // until every launch below has been enqueued
    std::copy(pw, pw + L + 1, g->pw);
    std::copy(ph, ph + L + 1, g->ph);
    std::copy(at, at + L + 1, g->at);
    g->last_stream = s;
    if (L == 0) {
        BT_HIP(bt_launch_glare_mean(rgba_device, samples, p.max_value, out_device, (uint64_t)width * height, s));
        return 0;
    }
    float w[BT_GLARE_MAX_LEVELS + 1];
    btglare::level_weights(L, p.spread, w);
    // down: A_L = D_L * w_L leaves the last of these kernels, so a call is 2 L launches
    BT_HIP(bt_launch_glare_down0(rgba_device, samples, p.max_value, width, height, g->plane(1), pw[1], ph[1], L == 1 ? w[1] : 1.0f, s));
    for (uint32_t k = 2; k <= L; ++k)
        BT_HIP(bt_launch_glare_down(g->plane(k - 1), pw[k - 1], ph[k - 1], g->plane(k), pw[k], ph[k], k == L ? w[L] : 1.0f, s));
    for (uint32_t k = L - 1; k >= 1; --k)
        BT_HIP(bt_launch_glare_up(g->plane(k), pw[k], ph[k], g->plane(k + 1), pw[k + 1], ph[k + 1], w[k], s));
    BT_HIP(bt_launch_glare_composite(rgba_device, samples, p.max_value, p.strength, g->plane(1), pw[1], ph[1], out_device, width, height,
                                     s));
    g->L = L;
    return 0;
}

int bt_debug_glare_plane(bt_glare *g, uint32_t level, float *host, uint32_t n) {
    if (!g) return fail(BT_ERR_INVALID_ARG, "null glare handle");
    if (level < 1 || level > g->L || !g->planes)
        return fail(BT_ERR_INVALID_ARG, "level " + std::to_string(level) + ": the last call has the planes 1 .. " + std::to_string(g->L));
    const uint64_t count = (uint64_t)g->pw[level] * g->ph[level] * 4;
    if (count > 0x7fffffffull) return fail(BT_ERR_INVALID_ARG, "the plane has more elements than the return value can count");
    if (n == 0) return (int)count;
    if (!host) return fail(BT_ERR_INVALID_ARG, "null buffer");
    n = (uint32_t)std::min<uint64_t>(n, count);
    BT_HIP(hipStreamSynchronize(g->last_stream));
    BT_HIP(hipMemcpy(host, g->plane(level), (size_t)n * 4, hipMemcpyDeviceToHost));
    return (int)n;
}

int bt_debug_glare_host(const float *rgba_host, uint32_t samples, float *out_host, uint32_t width, uint32_t height,
                        const bt_glare_params *params) {
    bt_glare_params p;
    if (params) p = *params;
    else bt_glare_params_default(&p);
    int rc = check_args(nullptr, rgba_host, samples, out_host, width, height, p, false);
    if (rc) return rc;
    static_assert(sizeof(btglare::Texel) == 16, "a texel is four floats");
    btglare::run_host((const btglare::Texel *)rgba_host, samples, (btglare::Texel *)out_host, width, height, p.levels, p.spread, p.strength,
                      p.max_value);
    return 0;
}

} // extern "C"
