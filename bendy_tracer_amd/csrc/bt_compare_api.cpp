// bt_compare_api.cpp -- EXTENSION, NOT IN THE REFERENCE: the C ABI of the compare stage (include/bendy_hip.h, bt_compare;
// DESIGN.md 20).  Validation, the handle's planes, slab and histograms, the launches and the frame sums, which are formed here on
// the host from the copied slab in tile order; the kernels are in bt_compare.hip, the definition in bt_compare.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/bendy_hip.h"
#include "bt_internal.hpp"
#include "bt_scene.hpp"
#define BT_COMPARE_LAUNCHERS
#include "bt_compare.hpp"

#pragma STDC FP_CONTRACT OFF

struct bt_compare {
    int device = -1;
    char *planes = nullptr;              // E (4 B), then (vx, vy) (16 B), then s (8 B) per pixel: the wide ones first in memory
    size_t capacity = 0;                 // pixels
    char *slab = nullptr;
    size_t slab_tiles = 0;
    uint32_t *hist = nullptr;            // three passes of BT_COMPARE_BINS
    std::vector<char> host_slab;
    // the last device call
    uint32_t w = 0, h = 0;
    bool called = false, polled = false;
    btcompare::Sums sums;
    double peak = 1.0;
    hipStream_t last_stream = nullptr;

    double *V() const { return (double *)planes; }
    double *S() const { return (double *)(planes + capacity * 16); }
    float *E() const { return (float *)(planes + capacity * 24); }
    size_t tiles() const { return (size_t)btcompare::tiles_of(w) * btcompare::tiles_of(h); }

    bool holds() const { return planes || slab || hist; }
    void release() {
        if (planes) (void)hipFree(planes);
        planes = nullptr;
        capacity = 0;
        if (slab) (void)hipFree(slab);
        slab = nullptr;
        slab_tiles = 0;
        if (hist) (void)hipFree(hist);
        hist = nullptr;
        called = polled = false;
    }
    ~bt_compare() {
        if (device >= 0 && holds()) {
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
        if (device >= 0 && device != dev_now && holds()) {
            (void)hipSetDevice(device);
            release();
            BT_HIP(hipSetDevice(dev_now));
        }
        device = dev_now;
        return 0;
    }
    // the slab on the host, after the stream has drained
    int fetch(BtCompareSlab &out) {
        const size_t n = tiles();
        host_slab.resize(n * BT_COMPARE_SLAB_BYTES);
        BT_HIP(hipStreamSynchronize(last_stream));
        BT_HIP(hipMemcpy(host_slab.data(), slab, n * BT_COMPARE_SLAB_BYTES, hipMemcpyDeviceToHost));
        out = bt_compare_slab(host_slab.data(), n);
        return 0;
    }
};

namespace {

bool bad_frame(uint32_t w, uint32_t h) {
    return w == 0 || h == 0 || (uint64_t)w * h > 0xffffffffull || w > 0x7fffffffu || h > 0x7fffffffu;
}

int check_args(const void *handle, const float *test, uint32_t test_samples, const float *ref, uint32_t ref_samples, uint32_t w, uint32_t h,
               const bt_compare_params *p, bool with_handle) {
    // in the order the header gives
    if ((with_handle && !handle) || !test || !ref || !p) return fail(BT_ERR_INVALID_ARG, "null compare handle, frame or params");
    if (test_samples == 0 || ref_samples == 0) return fail(BT_ERR_INVALID_ARG, "a frame with 0 samples");
    if (bad_frame(w, h)) return fail(BT_ERR_INVALID_ARG, "zero-sized or too large a frame");
    if (!std::isfinite(p->epsilon) || !(p->epsilon > 0.0)) return fail(BT_ERR_INVALID_ARG, "bt_compare_params.epsilon must be finite and > 0");
    if (!std::isfinite(p->peak) || !(p->peak > 0.0)) return fail(BT_ERR_INVALID_ARG, "bt_compare_params.peak must be finite and > 0");
    return 0;
}

void finish(const btcompare::Sums &s, double peak, bt_compare_stats *out) {
    out->pixels = s.pixels;
    out->valid = s.valid;
    out->nonfinite = s.nonfinite;
    out->max_index = s.max_index;
    out->mse = s.valid ? s.se / (double)(3 * s.valid) : 0.0;
    out->rel_mse = s.valid ? s.re / (double)(3 * s.valid) : 0.0;
    out->ssim = s.s / (double)s.pixels;
    out->max_abs = s.max_abs;
    out->psnr = out->mse == 0.0 ? (double)INFINITY : 10.0 * std::log10(peak * peak / out->mse);
}

bool bad_fraction(double f) { return !(f > 0.0) || !(f <= 1.0); }

} // namespace

extern "C" {

void bt_compare_params_default(bt_compare_params *out) {
    if (!out) return;
    out->epsilon = 0.01;                 // the relMSE of DESIGN.md 11 and of every table since
    out->peak = 1.0;
}

bt_compare *bt_compare_new(void) { return new bt_compare(); }

void bt_compare_free(bt_compare *h) { delete h; }

int bt_compare_device(bt_compare *h, const float *test_device, uint32_t test_samples, const float *ref_device, uint32_t ref_samples,
                      uint32_t width, uint32_t height, const bt_compare_params *params, void *stream) {
    int rc = check_args(h, test_device, test_samples, ref_device, ref_samples, width, height, params, true);
    if (rc) return rc;
    rc = h->bind();                      // BT_ERR_DEVICE without a device
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    h->called = h->polled = false;       // until both launches have been enqueued
    const size_t pixels = (size_t)width * height, tiles = (size_t)btcompare::tiles_of(width) * btcompare::tiles_of(height);
    if (pixels > h->capacity) {
        if (h->planes) (void)hipFree(h->planes);     // hipFree waits for the work that still uses the old planes
        h->planes = nullptr;
        h->capacity = 0;
        BT_HIP(hipMalloc((void **)&h->planes, pixels * 28));
        h->capacity = pixels;
    }
    if (tiles > h->slab_tiles) {
        if (h->slab) (void)hipFree(h->slab);
        h->slab = nullptr;
        h->slab_tiles = 0;
        BT_HIP(hipMalloc((void **)&h->slab, tiles * BT_COMPARE_SLAB_BYTES));
        h->slab_tiles = tiles;
    }
    if (!h->hist) BT_HIP(hipMalloc((void **)&h->hist, 3 * BT_COMPARE_BINS * sizeof(uint32_t)));
    h->w = width;
    h->h = height;
    h->last_stream = s;
    const BtCompareSlab slab = bt_compare_slab(h->slab, tiles);
    BT_HIP(bt_launch_compare_point(test_device, 1.0f / (float)test_samples, ref_device, 1.0f / (float)ref_samples, width, height,
                                   params->epsilon, h->E(), h->V(), slab, s));
    BT_HIP(bt_launch_compare_ssim(h->V(), width, height, h->S(), slab, s));
    h->peak = params->peak;
    h->called = true;
    return 0;
}

int bt_compare_poll(bt_compare *h, bt_compare_stats *out) {
    if (!h || !out) return fail(BT_ERR_INVALID_ARG, "null compare handle or stats");
    if (!h->called) return fail(BT_ERR_INVALID_ARG, "bt_compare_poll before a bt_compare_device call");
    if (!h->polled) {
        BtCompareSlab b;
        int rc = h->fetch(b);
        if (rc) return rc;
        const size_t n = h->tiles();
        btcompare::Sums s;
        s.pixels = (uint64_t)h->w * h->h;
        s.se = btcompare::ordered_sum(b.se, n);
        s.re = btcompare::ordered_sum(b.re, n);
        s.s = btcompare::ordered_sum(b.s, n);
        s.max_index = 0xffffffffu;
        for (size_t t = 0; t < n; ++t) {
            s.valid += b.valid[t];
            s.nonfinite += b.nonfinite[t];
            btcompare::max_merge(s.max_abs, s.max_index, b.m[t], b.index[t]);
        }
        h->sums = s;
        h->polled = true;
    }
    finish(h->sums, h->peak, out);
    return 0;
}

int bt_compare_tail(bt_compare *h, double fraction, double *share, float *threshold) {
    if (!h) return fail(BT_ERR_INVALID_ARG, "null compare handle");
    if (bad_fraction(fraction)) return fail(BT_ERR_INVALID_ARG, "the tail's fraction must lie in (0, 1]");
    if (!h->called) return fail(BT_ERR_INVALID_ARG, "bt_compare_tail before a bt_compare_device call");
    bt_compare_stats st;
    int rc = bt_compare_poll(h, &st);    // `valid`
    if (rc) return rc;
    double sh = 0.0;
    float T = 0.0f;
    if (st.valid) {
        const uint64_t k0 = btcompare::tail_rank(fraction, st.valid);
        uint64_t k = k0;
        uint32_t prefix = 0;
        uint32_t bins[BT_COMPARE_BINS];
        hipStream_t s = h->last_stream;
        const uint32_t n = (uint32_t)((uint64_t)h->w * h->h);
        BT_HIP(hipMemsetAsync(h->hist, 0, 3 * BT_COMPARE_BINS * sizeof(uint32_t), s));
        for (int pass = 0; pass < 3; ++pass) {
            uint32_t *hist = h->hist + pass * BT_COMPARE_BINS;
            BT_HIP(bt_launch_compare_hist(h->E(), n, btcompare::kPassShift[pass], btcompare::kPassPrefixShift[pass], prefix, hist, s));
            BT_HIP(hipStreamSynchronize(s));
            BT_HIP(hipMemcpy(bins, hist, sizeof bins, hipMemcpyDeviceToHost));
            const uint32_t b = btcompare::select_bin(bins, k);
            prefix = (prefix << (btcompare::kPassPrefixShift[pass] - btcompare::kPassShift[pass])) | b;
        }
        __builtin_memcpy(&T, &prefix, 4);
        const size_t tiles = h->tiles();
        BT_HIP(bt_launch_compare_tail(h->E(), h->w, h->h, T, bt_compare_slab(h->slab, tiles), s));
        BtCompareSlab b;
        rc = h->fetch(b);
        if (rc) return rc;
        uint64_t c_gt = 0;
        for (size_t t = 0; t < tiles; ++t) c_gt += b.c_gt[t];
        sh = btcompare::tail_share(btcompare::ordered_sum(b.gt, tiles), btcompare::ordered_sum(b.all, tiles), c_gt, k0, T);
    }
    if (share) *share = sh;
    if (threshold) *threshold = T;
    return 0;
}

int bt_compare_map_device(bt_compare *h, uint8_t *rgba8_device, float scale, void *stream) {
    if (!h || !rgba8_device) return fail(BT_ERR_INVALID_ARG, "null compare handle or output");
    if (!std::isfinite(scale) || !(scale > 0.0f)) return fail(BT_ERR_INVALID_ARG, "the map's scale must be finite and > 0");
    if (!h->called) return fail(BT_ERR_INVALID_ARG, "bt_compare_map_device before a bt_compare_device call");
    BT_HIP(bt_launch_compare_map(h->E(), (uint32_t)((uint64_t)h->w * h->h), scale, rgba8_device, (hipStream_t)stream));
    return 0;
}

int bt_debug_compare_plane(bt_compare *h, uint32_t which, void *host, uint32_t n) {
    if (!h) return fail(BT_ERR_INVALID_ARG, "null compare handle");
    if (which > 2u) return fail(BT_ERR_INVALID_ARG, "plane " + std::to_string(which) + ": 0 is E, 1 is (vx, vy), 2 is s");
    if (!h->called || !h->planes) return fail(BT_ERR_INVALID_ARG, "the handle has no planes: there has been no device call");
    const uint64_t per = which == 1u ? 2 : 1, count = (uint64_t)h->w * h->h * per;
    if (count > 0x7fffffffull) return fail(BT_ERR_INVALID_ARG, "the plane has more elements than the return value can count");
    if (n == 0) return (int)count;
    if (!host) return fail(BT_ERR_INVALID_ARG, "null buffer");
    if (n > count) n = (uint32_t)count;
    BT_HIP(hipStreamSynchronize(h->last_stream));
    const void *src = which == 0u ? (const void *)h->E() : which == 1u ? (const void *)h->V() : (const void *)h->S();
    BT_HIP(hipMemcpy(host, src, (size_t)n * (which == 0u ? 4 : 8), hipMemcpyDeviceToHost));
    return (int)n;
}

int bt_debug_compare_host(const float *test_host, uint32_t test_samples, const float *ref_host, uint32_t ref_samples, uint32_t width,
                          uint32_t height, const bt_compare_params *params, bt_compare_stats *stats, float *e_host, double *v_host,
                          double *s_host, uint32_t n_tail, const double *fractions, double *shares, float *thresholds) {
    int rc = check_args(nullptr, test_host, test_samples, ref_host, ref_samples, width, height, params, false);
    if (rc) return rc;
    if (n_tail && (!fractions || !shares || !thresholds)) return fail(BT_ERR_INVALID_ARG, "a tail is asked for without its arrays");
    for (uint32_t i = 0; i < n_tail; ++i)
        if (bad_fraction(fractions[i])) return fail(BT_ERR_INVALID_ARG, "the tail's fraction must lie in (0, 1]");
    static_assert(sizeof(btcompare::Texel) == 16 && sizeof(btcompare::Pair) == 16, "a texel is four floats, a pair two doubles");
    const size_t pixels = (size_t)width * height;
    std::vector<float> E(e_host ? 0 : pixels);
    std::vector<btcompare::Pair> V(v_host ? 0 : pixels);
    std::vector<double> S(s_host ? 0 : pixels);
    float *e = e_host ? e_host : E.data();
    btcompare::Sums sums;
    btcompare::run_host((const btcompare::Texel *)test_host, test_samples, (const btcompare::Texel *)ref_host, ref_samples, width, height,
                        params->epsilon, e, v_host ? (btcompare::Pair *)v_host : V.data(), s_host ? s_host : S.data(), sums);
    if (stats) finish(sums, params->peak, stats);
    for (uint32_t i = 0; i < n_tail; ++i) btcompare::tail_host(e, width, height, sums.valid, fractions[i], shares[i], thresholds[i]);
    return 0;
}

int bt_read_pfm(const char *path, float *rgba_host, size_t capacity_floats, uint32_t *width, uint32_t *height) {
    if (!path || !width || !height) return fail(BT_ERR_INVALID_ARG, "null path, width or height");
    try {
        bt::read_pfm(path, rgba_host, capacity_floats, *width, *height);
        return 0;
    } catch (const bt::Error &e) {
        return fail(e.code, e.message);
    }
}

} // extern "C"
