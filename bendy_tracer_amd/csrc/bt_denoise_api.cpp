// bt_denoise_api.cpp -- EXTENSION, NOT IN THE REFERENCE: the C ABI of the AOV-guided a-trous denoiser (include/bendy_hip.h,
// bt_denoiser).  Validation, the handle's scratch and the host-buffer path; the kernels are in bt_denoise.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/bendy_hip.h"
#include "bt_internal.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr uint32_t kMaxLevels = 10;

// Everything that can be checked without the device.  Returns 0 or BT_ERR_INVALID_ARG (with bt_last_error set).
int validate(const bt_denoiser *d, const float *color, uint32_t color_samples, const float *albedo, uint32_t albedo_samples,
             const float *normal, uint32_t normal_samples, const float *depth, uint32_t depth_samples, const float *out,
             uint32_t width, uint32_t height, const bt_denoise_params &p) {
    if (!d) return fail(BT_ERR_INVALID_ARG, "null denoiser");
    if (!color || !out) return fail(BT_ERR_INVALID_ARG, "null colour or output buffer");
    if (width == 0 || height == 0) return fail(BT_ERR_INVALID_ARG, "zero-sized buffer");
    if ((size_t)width * height > 0x7fffffffu) return fail(BT_ERR_INVALID_ARG, "buffer too large");
    if (color_samples == 0) return fail(BT_ERR_INVALID_ARG, "colour buffer with 0 samples");
    if (albedo && albedo_samples == 0) return fail(BT_ERR_INVALID_ARG, "albedo buffer with 0 samples");
    if (normal && normal_samples == 0) return fail(BT_ERR_INVALID_ARG, "normal buffer with 0 samples");
    if (depth && depth_samples == 0) return fail(BT_ERR_INVALID_ARG, "depth buffer with 0 samples");
    if (p.levels > kMaxLevels) return fail(BT_ERR_INVALID_ARG, "bt_denoise_params.levels must be 0 .. 10");
    if (!std::isfinite(p.sigma_color) || !(p.sigma_color > 0.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_denoise_params.sigma_color must be finite and > 0");
    if (!std::isfinite(p.sigma_depth) || !(p.sigma_depth > 0.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_denoise_params.sigma_depth must be finite and > 0");
    if (!std::isfinite(p.sigma_normal) || !(p.sigma_normal >= 0.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_denoise_params.sigma_normal must be finite and >= 0");
    if (!std::isfinite(p.eps_albedo) || !(p.eps_albedo >= 0.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_denoise_params.eps_albedo must be finite and >= 0");
    if (out == color || out == albedo || out == normal || out == depth)
        return fail(BT_ERR_INVALID_ARG, "out must not alias an input: the inputs are running sums, out is a mean");
    return 0;
}

} // namespace

struct bt_denoiser {
    int device = -1;
    float *scratch = nullptr;      // e0 | e1 | guide, `pixels` float4 each (48 B per pixel)
    size_t pixels = 0;
    float *io = nullptr;           // bt_denoise: device copies of the host buffers (colour, albedo, normal, depth, out)
    size_t io_pixels = 0;

    void release() {
        if (scratch) (void)hipFree(scratch);
        if (io) (void)hipFree(io);
        scratch = io = nullptr;
        pixels = io_pixels = 0;
    }
    ~bt_denoiser() {
        if (device >= 0 && (scratch || io)) {
            int cur = -1;
            if (hipGetDevice(&cur) == hipSuccess && cur != device) (void)hipSetDevice(device);
            release();
            if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
        }
    }
    // Binds the handle to the current device; memory held for another device is returned there first.
    int bind() {
        int dev = -1;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return hip_fail("hipGetDevice", e);
        if (device >= 0 && device != dev) {
            (void)hipSetDevice(device);
            release();
            e = hipSetDevice(dev);
            if (e != hipSuccess) return hip_fail("hipSetDevice", e);
        }
        device = dev;
        return 0;
    }
    // Grows (never shrinks) a block of `planes` float4 planes of `n` pixels.  hipFree waits for the work still reading it.
    static int grow(float *&ptr, size_t &have, size_t n, size_t planes) {
        if (have >= n) return 0;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        have = 0;
        hipError_t e = hipMalloc((void **)&ptr, n * planes * 16);
        if (e != hipSuccess) return hip_fail("hipMalloc (denoiser scratch)", e);
        have = n;
        return 0;
    }
};

extern "C" {

void bt_denoise_params_default(bt_denoise_params *out) {
    if (!out) return;
    // tuned on cornell / scene / volume at 4 spp against 1024-spp renders, 128x128 and 768x512
    out->levels = 2;
    out->sigma_color = 16.0f;
    out->sigma_normal = 16.0f;
    out->sigma_depth = 1.0f;
    out->eps_albedo = 1e-3f;
}

bt_denoiser *bt_denoiser_new(void) { return new bt_denoiser(); }

void bt_denoiser_free(bt_denoiser *d) { delete d; }

int bt_denoise_device(bt_denoiser *d, const float *color, uint32_t color_samples, const float *albedo,
                      uint32_t albedo_samples, const float *normal, uint32_t normal_samples, const float *depth,
                      uint32_t depth_samples, float *out, uint32_t width, uint32_t height, const bt_denoise_params *params,
                      void *stream) {
    bt_denoise_params p;
    if (params) p = *params;
    else bt_denoise_params_default(&p);
    int rc = validate(d, color, color_samples, albedo, albedo_samples, normal, normal_samples, depth, depth_samples, out,
                      width, height, p);
    if (rc) return rc;
    rc = d->bind();
    if (rc) return rc;
    const size_t n = (size_t)width * height;
    if (p.levels > 0) {
        rc = bt_denoiser::grow(d->scratch, d->pixels, n, 3);
        if (rc) return rc;
    }
    float *e0 = d->scratch, *e1 = e0 ? e0 + 4 * n : nullptr, *guide = e0 ? e0 + 8 * n : nullptr;
    hipError_t e = bt_launch_denoise(color, (float)color_samples, albedo, (float)albedo_samples, normal,
                                     (float)normal_samples, depth, (float)depth_samples, out, e0, e1, guide, width, height,
                                     p.levels, p.sigma_color, p.sigma_normal, p.sigma_depth, p.eps_albedo,
                                     (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("bt_denoise kernels", e);
    return 0;
}

int bt_denoise(bt_denoiser *d, const float *color, uint32_t color_samples, const float *albedo, uint32_t albedo_samples,
               const float *normal, uint32_t normal_samples, const float *depth, uint32_t depth_samples, float *out,
               uint32_t width, uint32_t height, const bt_denoise_params *params) {
    bt_denoise_params p;
    if (params) p = *params;
    else bt_denoise_params_default(&p);
    int rc = validate(d, color, color_samples, albedo, albedo_samples, normal, normal_samples, depth, depth_samples, out,
                      width, height, p);
    if (rc) return rc;
    rc = d->bind();
    if (rc) return rc;
    const size_t n = (size_t)width * height, bytes = n * 16;
    rc = bt_denoiser::grow(d->io, d->io_pixels, n, 5);
    if (rc) return rc;
    float *dev[5];
    for (int i = 0; i < 5; ++i) dev[i] = d->io + (size_t)i * 4 * n;
    const float *host[4] = {color, albedo, normal, depth};
    for (int i = 0; i < 4; ++i) {
        if (!host[i]) {
            dev[i] = nullptr;
            continue;
        }
        hipError_t e = hipMemcpyAsync(dev[i], host[i], bytes, hipMemcpyHostToDevice, nullptr);
        if (e != hipSuccess) return hip_fail("hipMemcpyAsync", e);
    }
    rc = bt_denoise_device(d, dev[0], color_samples, dev[1], albedo_samples, dev[2], normal_samples, dev[3], depth_samples,
                           dev[4], width, height, &p, nullptr);
    if (rc) return rc;
    hipError_t e = hipMemcpy(out, dev[4], bytes, hipMemcpyDeviceToHost);       // stream-ordered behind the kernels
    if (e != hipSuccess) return hip_fail("hipMemcpy", e);
    return 0;
}

} // extern "C"
