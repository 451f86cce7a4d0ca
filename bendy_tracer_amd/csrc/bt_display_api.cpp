// bt_display_api.cpp -- EXTENSION, NOT IN THE REFERENCE: the C ABI of the display stage (include/bendy_hip.h, bt_display;
// DESIGN.md 15).  Validation and the handle's device words; the kernels are in bt_display.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/bendy_hip.h"
#include "bt_internal.hpp"

#pragma STDC FP_CONTRACT OFF

struct bt_display {
    int device = -1;
    // one allocation: live counters | the last call's counters | BtDisplayState
    uint32_t *words = nullptr;
    bool clear_pending = true;     // the words are zeroed on the stream of the next call (fresh allocation, bt_display_reset)
    bool shown = false;            // a call since _new / _reset has written shown_ev / shown_mult
    bool metered = false;          // ... and one of them has written the last call's counters
    hipStream_t last_stream = nullptr;

    static constexpr size_t kBytes = 2 * BT_DISPLAY_STRIDE * 4 + sizeof(BtDisplayState);
    uint32_t *live() const { return words; }
    uint32_t *last() const { return words + BT_DISPLAY_STRIDE; }
    BtDisplayState *state() const { return (BtDisplayState *)(words + 2 * BT_DISPLAY_STRIDE); }
    void release() {
        if (words) (void)hipFree(words);
        words = nullptr;
    }
    ~bt_display() {
        if (device >= 0 && words) {
            int c = -1;
            if (hipGetDevice(&c) == hipSuccess && c != device) (void)hipSetDevice(device);
            release();
            if (c >= 0 && c != device) (void)hipSetDevice(c);
        }
    }
    // The words on the current device (a handle that held some on another device starts afresh).
    int ensure() {
        int dev = -1;
        BT_HIP(hipGetDevice(&dev));
        if (words && device != dev) {
            (void)hipSetDevice(device);
            release();
            BT_HIP(hipSetDevice(dev));
        }
        device = dev;
        if (words) return 0;
        BT_HIP(hipMalloc((void **)&words, kBytes));
        clear_pending = true;
        shown = metered = false;
        return 0;
    }
};

namespace {

int check_params(const bt_display_params &p) {
    if (p.tonemap != BT_TONEMAP_CLIP && p.tonemap != BT_TONEMAP_REINHARD && p.tonemap != BT_TONEMAP_ACES)
        return fail(BT_ERR_INVALID_ARG, "bt_display_params.tonemap " + std::to_string(p.tonemap) + " is no operator");
    if (!std::isfinite(p.ev)) return fail(BT_ERR_INVALID_ARG, "bt_display_params.ev must be finite");
    if (!std::isfinite(p.key) || !(p.key > 0.0)) return fail(BT_ERR_INVALID_ARG, "bt_display_params.key must be finite and > 0");
    if (!(p.p_low >= 0.0f && p.p_low < 1.0f) || !(p.p_high >= 0.0f && p.p_high < 1.0f) || !(p.p_low + p.p_high < 1.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_display_params.p_low and p_high must be in [0, 1) with p_low + p_high < 1");
    if (!(p.adapt > 0.0f && p.adapt <= 1.0f)) return fail(BT_ERR_INVALID_ARG, "bt_display_params.adapt must be in (0, 1]");
    if (!(p.ev_min <= p.ev_max)) return fail(BT_ERR_INVALID_ARG, "bt_display_params.ev_min must not exceed ev_max");
    if (!(p.white > 0.0f)) return fail(BT_ERR_INVALID_ARG, "bt_display_params.white must be > 0");
    return 0;
}

} // namespace

extern "C" {

void bt_display_params_default(bt_display_params *out) {
    if (!out) return;
    // starting values: a photographic 18 % key over the frame's 10th to 98th percentile
    out->tonemap = BT_TONEMAP_ACES;
    out->auto_exposure = 1;
    out->ev = 0.0f;
    out->key = 0.18;
    out->p_low = 0.10f;
    out->p_high = 0.02f;
    out->adapt = 1.0f;
    out->ev_min = -8.0f;
    out->ev_max = 8.0f;
    out->white = 4.0f;
}

bt_display *bt_display_new(void) { return new bt_display(); }

void bt_display_free(bt_display *d) { delete d; }

int bt_display_reset(bt_display *d) {
    if (!d) return fail(BT_ERR_INVALID_ARG, "null display handle");
    d->clear_pending = true;       // the next call zeroes the counters and the state on its stream
    d->shown = d->metered = false;
    return 0;
}

int bt_display_device(bt_display *d, const float *rgba_device, uint32_t samples, uint8_t *rgba8_device, uint32_t width,
                      uint32_t height, int32_t color_space, const bt_display_params *params, void *stream) {
    // everything that can be refused is refused before the device is touched, in the order the header gives
    if (!d || !rgba_device || !rgba8_device) return fail(BT_ERR_INVALID_ARG, "null display handle, input or output buffer");
    if (samples == 0) return fail(BT_ERR_INVALID_ARG, "frame with 0 samples");
    if (width == 0 || height == 0 || (uint64_t)width * height > 0xffffffffull)
        return fail(BT_ERR_INVALID_ARG, "zero-sized or too large a frame");
    if ((const void *)rgba_device == (const void *)rgba8_device)
        return fail(BT_ERR_INVALID_ARG, "the output must not alias the input: the input is RGBA32F, the output RGBA8");
    if (color_space != BT_COLOR_NONE && color_space != BT_COLOR_LINEAR && color_space != BT_COLOR_SRGB)
        return fail(BT_ERR_INVALID_ARG, "colour space " + std::to_string(color_space) +
                                            ": the display stage takes NONE, LINEAR or SRGB (NORMAL is for the normal AOV)");
    bt_display_params p;
    if (params) p = *params;
    else bt_display_params_default(&p);
    int rc = check_params(p);
    if (rc) return rc;

    rc = d->ensure();
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (d->clear_pending) {
        BT_HIP(hipMemsetAsync(d->words, 0, bt_display::kBytes, s));
        d->clear_pending = false;
    }
    const uint64_t n = (uint64_t)width * height;
    if (p.auto_exposure) {
        BtDisplayExpose x{};
        x.log2_key = std::log2(p.key);
        x.p_low = p.p_low;
        x.p_high = p.p_high;
        x.ev = p.ev;
        x.ev_min = p.ev_min;
        x.ev_max = p.ev_max;
        x.adapt = p.adapt;
        BT_HIP(bt_launch_display_meter(rgba_device, n, samples, d->live(), s));
        BT_HIP(bt_launch_display_expose(d->live(), d->last(), d->state(), &x, s));
        d->metered = true;
    }
    const float iw2 = 1.0f / (p.white * p.white);
    BT_HIP(bt_launch_display_show(rgba_device, rgba8_device, n, samples, color_space, p.tonemap, iw2, !p.auto_exposure, p.ev,
                                  d->state(), s));
    d->shown = true;
    d->last_stream = s;
    return 0;
}

int bt_display_exposure(bt_display *d, float *ev, float *mult) {
    if (!d) return fail(BT_ERR_INVALID_ARG, "null display handle");
    if (!d->shown || !d->words) return fail(BT_ERR_INVALID_ARG, "no frame has been displayed since bt_display_new / bt_display_reset");
    BtDisplayState st;
    BT_HIP(hipStreamSynchronize(d->last_stream));
    BT_HIP(hipMemcpy(&st, d->state(), sizeof st, hipMemcpyDeviceToHost));
    if (ev) *ev = st.shown_ev;
    if (mult) *mult = st.shown_mult;
    return 0;
}

int bt_debug_display_histogram(bt_display *d, uint32_t *host, uint32_t n) {
    if (!d) return fail(BT_ERR_INVALID_ARG, "null display handle");
    if (n == 0) return BT_DISPLAY_COUNTERS;
    if (!host) return fail(BT_ERR_INVALID_ARG, "null buffer");
    n = std::min<uint32_t>(n, BT_DISPLAY_COUNTERS);
    if (!d->metered || !d->words) {
        std::fill(host, host + n, 0u);
        return (int)n;
    }
    BT_HIP(hipStreamSynchronize(d->last_stream));
    BT_HIP(hipMemcpy(host, d->last(), (size_t)n * 4, hipMemcpyDeviceToHost));
    return (int)n;
}

} // extern "C"
