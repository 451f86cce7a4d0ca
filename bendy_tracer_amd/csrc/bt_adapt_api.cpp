// bt_adapt_api.cpp -- EXTENSION, NOT IN THE REFERENCE: the C ABI of variance-driven adaptive sampling (include/bendy_hip.h,
// bt_adaptive).  Validation and the handle's buffers; the render half is bt_api.cpp's render_common with the
// OUTPUT == 5 builds of bt_kernels.hip, the update and resolve kernels are in bt_adapt.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/bendy_hip.h"
#include "bt_internal.hpp"
#include "bt_plan.hpp"

struct bt_adaptive {
    uint32_t width = 0, height = 0, tiles_x = 0, tiles_y = 0;
    int device = -1;
    // one allocation: moment plane (pixels floats) | count | active | error (tiles words each) | the active-tile counter
    float *d_moment = nullptr;
    uint32_t *d_count = nullptr, *d_active = nullptr, *d_n_active = nullptr;
    float *d_error = nullptr;
    bool fresh = true;             // reset since the last pass: the device buffers (if any) are yet to be cleared
    bool done = false;             // a poll has found no tile active
    uint32_t next_sample = 0;      // sample index of the next pass's first sample
    uint32_t samples = 0, subsample_n = 0;   // the pass size since the reset; samples == 0: none yet
    uint32_t passes = 0;
    hipStream_t last_stream = nullptr;

    uint32_t tiles() const { return tiles_x * tiles_y; }
    size_t pixels() const { return (size_t)width * height; }
    void release() {
        if (d_moment) (void)hipFree(d_moment);
        d_moment = d_error = nullptr;
        d_count = d_active = d_n_active = nullptr;
    }
    ~bt_adaptive() {
        if (device >= 0 && d_moment) {
            int cur = -1;
            if (hipGetDevice(&cur) == hipSuccess && cur != device) (void)hipSetDevice(device);
            release();
            if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
        }
    }
    // Buffers on the current device (a handle that held some on another device starts afresh: their contents are gone).
    int ensure() {
        int dev = -1;
        BT_HIP(hipGetDevice(&dev));
        if (d_moment && device != dev) {
            (void)hipSetDevice(device);
            release();
            BT_HIP(hipSetDevice(dev));
            fresh = true;
        }
        device = dev;
        if (d_moment) return 0;
        const size_t words = pixels() + 3 * (size_t)tiles() + 1;
        BT_HIP(hipMalloc((void **)&d_moment, words * 4));
        d_count = (uint32_t *)(d_moment + pixels());
        d_active = d_count + tiles();
        d_error = (float *)(d_active + tiles());
        d_n_active = (uint32_t *)(d_error + tiles());
        fresh = true;
        return 0;
    }
    int clear(hipStream_t stream) {
        BT_HIP(hipMemsetAsync(d_moment, 0, (pixels() + 3 * (size_t)tiles() + 1) * 4, stream));
        BT_HIP(hipMemsetD32Async((hipDeviceptr_t)d_active, 1, tiles(), stream));
        fresh = false;
        return 0;
    }
    // `n` words from `src` to the host behind the last pass; zeros while nothing has been rendered since the reset
    int fetch(const void *src, void *host, uint32_t n) {
        if (fresh || !d_moment) {
            std::fill((uint32_t *)host, (uint32_t *)host + n, 0u);
            return 0;
        }
        BT_HIP(hipStreamSynchronize(last_stream));
        BT_HIP(hipMemcpy(host, src, (size_t)n * 4, hipMemcpyDeviceToHost));
        return 0;
    }
};

extern "C" {

void bt_adaptive_params_default(bt_adaptive_params *out) {
    if (!out) return;
    // chosen on scene / cornell2 / volume at 768x512 against uniform renders at the cap
    out->threshold = 0.02f;
    out->min_samples = 16;
    out->max_samples = 1024;
    out->eps = 1e-3f;
}

bt_adaptive *bt_adaptive_new(uint32_t width, uint32_t height) {
    if (width == 0 || height == 0 || (uint64_t)width * height > 0x7fffffffu) {
        fail(BT_ERR_INVALID_ARG, "bt_adaptive_new: zero-sized or too large a frame");
        return nullptr;
    }
    bt_adaptive *a = new bt_adaptive();
    a->width = width;
    a->height = height;
    a->tiles_x = btplan::tiles_across(width);
    a->tiles_y = btplan::tiles_across(height);
    return a;
}

void bt_adaptive_free(bt_adaptive *a) { delete a; }

int bt_adaptive_reset(bt_adaptive *a) {
    if (!a) return fail(BT_ERR_INVALID_ARG, "null adaptive handle");
    a->fresh = true;               // the next pass clears the buffers on its stream, ahead of its kernels
    a->done = false;
    a->next_sample = 0;
    a->samples = a->subsample_n = 0;
    a->passes = 0;
    return 0;
}

int bt_render_adaptive_device(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                              bt_adaptive *adaptive, const bt_adaptive_params *params, float *rgba_device, uint32_t width,
                              uint32_t height, uint64_t seed, void *stream) {
    // everything that can be refused is refused before the device is touched, in the order the header gives
    if (!scene || !config || !render || !adaptive || !params || !rgba_device) return fail(BT_ERR_INVALID_ARG, "null argument");
    const int output = render->has_output ? render->output : config->output;
    if (output != BT_OUTPUT_FULL)
        return fail(BT_ERR_INVALID_ARG, "an adaptive pass renders the Full output: the effective output must be BT_OUTPUT_FULL");
    bt_adaptive *a = adaptive;
    if (width != a->width || height != a->height)
        return fail(BT_ERR_INVALID_ARG, "frame of " + std::to_string(width) + "x" + std::to_string(height) + " on an adaptive handle of " +
                                            std::to_string(a->width) + "x" + std::to_string(a->height));
    if (!std::isfinite(params->threshold) || !(params->threshold >= 0.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_adaptive_params.threshold must be finite and >= 0");
    if (params->min_samples > params->max_samples)
        return fail(BT_ERR_INVALID_ARG, "bt_adaptive_params.min_samples must not exceed max_samples");
    const uint32_t n = render->subsample_n >= 2 ? render->subsample_n : 1;
    if (a->samples != 0 && (render->samples != a->samples || n != a->subsample_n))
        return fail(BT_ERR_INVALID_ARG, "samples / subsample_n differ from the handle's earlier passes (" + std::to_string(a->samples) +
                                            " x " + std::to_string(a->subsample_n) + "^2): bt_adaptive_reset first");
    if (bt_scene_lens_on_internal(scene)) return fail(BT_ERR_UNSUPPORTED, "the lens extension has no adaptive builds");
    if (render->samples == 0) return BT_DONE;                          // mod.rs:186-188
    if ((uint64_t)render->samples * n * n > 0x7fffffffu || (uint64_t)a->next_sample + render->samples > 0xffffffffull)
        return fail(BT_ERR_INVALID_ARG, "sample count overflows");
    if (a->done) return BT_DONE;                                       // the last poll found every tile stopped

    int rc = a->ensure();
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (a->fresh && (rc = a->clear(st)) != 0) return rc;
    bt_render_config r = *render;
    r.sample_base = a->next_sample;
    rc = bt_render_adaptive_pass_internal(scene, camera_ref, config, &r, rgba_device, width, height, seed, stream, a->d_active,
                                          a->d_moment);
    if (rc < 0) return rc;
    a->last_stream = st;
    // (a split render has issued all its parts by now: the tiles are judged once, on the whole pass)
    BT_HIP(hipMemsetAsync(a->d_n_active, 0, 4, st));
    BT_HIP(bt_launch_adapt_update(rgba_device, a->d_moment, a->d_count, a->d_active, a->d_error, a->d_n_active, width, height,
                                  render->samples * n * n, params, st));
    a->samples = render->samples;
    a->subsample_n = n;
    a->next_sample += render->samples;
    a->passes += 1;
    return BT_IN_PROGRESS;
}

int bt_adaptive_poll(bt_adaptive *a, bt_adaptive_stats *out) {
    if (!a) return fail(BT_ERR_INVALID_ARG, "null adaptive handle");
    bt_adaptive_stats s{};
    s.tiles = s.active_tiles = a->tiles();
    s.passes = a->passes;
    if (!a->fresh && a->d_moment) {
        std::vector<uint32_t> counts(a->tiles());
        int rc = a->fetch(a->d_count, counts.data(), a->tiles());
        if (rc) return rc;
        BT_HIP(hipMemcpy(&s.active_tiles, a->d_n_active, 4, hipMemcpyDeviceToHost));
        s.min_count = *std::min_element(counts.begin(), counts.end());
        s.max_count = *std::max_element(counts.begin(), counts.end());
        s.pixel_samples = btplan::pixels_owned(a->width, a->height, 0, 1, counts.data());
        a->done = s.active_tiles == 0;
    }
    if (out) *out = s;
    return s.active_tiles == 0 ? BT_DONE : BT_IN_PROGRESS;
}

int bt_adaptive_counts(bt_adaptive *a, uint32_t *host, uint32_t n) {
    if (!a) return fail(BT_ERR_INVALID_ARG, "null adaptive handle");
    if (n == 0) return (int)a->tiles();
    if (!host) return fail(BT_ERR_INVALID_ARG, "null buffer");
    n = std::min(n, a->tiles());
    const int rc = a->fetch(a->d_count, host, n);
    return rc ? rc : (int)n;
}

int bt_adaptive_errors(bt_adaptive *a, float *host, uint32_t n) {
    if (!a) return fail(BT_ERR_INVALID_ARG, "null adaptive handle");
    if (n == 0) return (int)a->tiles();
    if (!host) return fail(BT_ERR_INVALID_ARG, "null buffer");
    n = std::min(n, a->tiles());
    const int rc = a->fetch(a->d_error, host, n);
    return rc ? rc : (int)n;
}

int bt_debug_adaptive_moments(bt_adaptive *a, float *host, uint32_t n) {
    if (!a) return fail(BT_ERR_INVALID_ARG, "null adaptive handle");
    if (n == 0) return (int)a->pixels();
    if (!host) return fail(BT_ERR_INVALID_ARG, "null buffer");
    n = (uint32_t)std::min<size_t>(n, a->pixels());
    const int rc = a->fetch(a->d_moment, host, n);
    return rc ? rc : (int)n;
}

int bt_adaptive_resolve_device(bt_adaptive *a, const float *rgba_device, float *out_device, void *stream) {
    if (!a || !rgba_device || !out_device) return fail(BT_ERR_INVALID_ARG, "null argument");
    if (rgba_device == out_device) return fail(BT_ERR_INVALID_ARG, "out must not be rgba: rgba holds running sums, out is a mean");
    int rc = a->ensure();
    if (rc) return rc;
    if (a->fresh && (rc = a->clear((hipStream_t)stream)) != 0) return rc;
    BT_HIP(bt_launch_adapt_resolve(rgba_device, a->d_count, out_device, a->width, a->height, (hipStream_t)stream));
    return 0;
}

} // extern "C"
