// bt_upscale_api.cpp -- EXTENSION, NOT IN THE REFERENCE: the C ABI of the upscale stage (include/bendy_hip.h, bt_upscale;
// DESIGN.md 19).  Validation, the handle's tables, prepared planes and counters and the two launches; the kernels are in
// bt_upscale.hip, the definition in bt_upscale.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>

#include "../../include/bendy_hip.h"
#include "bt_internal.hpp"
#define BT_UPSCALE_LAUNCHERS
#include "bt_upscale.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

// one axis table's copy on the device: weights[dst][8], first[dst], nearest[dst] in one allocation (the weights first: they
// are read 16 bytes at a time)
struct DeviceAxis {
    char *mem = nullptr;
    size_t capacity = 0;                 // bytes
    uint32_t src = 0, dst = 0;           // what it holds (dst == 0: nothing)
    bool is(const btupscale::Axis &a) const { return dst != 0 && src == a.src && dst == a.dst; }
};

} // namespace

struct bt_upscale {
    int device = -1;
    btupscale::Axis axis[2];             // x, y: the tables of the last call (device or host), kept for the next
    DeviceAxis dev[2];
    float *planes = nullptr;             // three planes of w x h float4: (c.rgb, z), (n.xyz, 0), (a.rgb, 0)
    size_t capacity = 0;                 // in texels of one plane
    unsigned long long *counters = nullptr;      // tier 2 in the low word, tier 3 in the high one
    // the last device call
    uint32_t pw = 0, ph = 0, pixels = 0;
    bool called = false;
    hipStream_t last_stream = nullptr;
    bool in_flight = false;              // a device call has been enqueued since the last synchronisation the handle knows of

    bool holds() const { return planes || counters || dev[0].mem || dev[1].mem; }
    void release() {
        if (planes) (void)hipFree(planes);
        planes = nullptr;
        capacity = 0;
        if (counters) (void)hipFree(counters);
        counters = nullptr;
        for (DeviceAxis &d : dev) {
            if (d.mem) (void)hipFree(d.mem);
            d = DeviceAxis();
        }
        called = false;
        in_flight = false;
    }
    ~bt_upscale() {
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
    // the host table of axis `a`; an upload of the table it replaces may still be reading it
    int table(int a, uint32_t src, uint32_t dst) {
        if (axis[a].is(src, dst)) return 0;
        if (in_flight) {
            BT_HIP(hipStreamSynchronize(last_stream));
            in_flight = false;
        }
        btupscale::build_axis(axis[a], src, dst);
        return 0;
    }
    int upload(int a, hipStream_t s, BtUpscaleAxis &out) {
        const btupscale::Axis &t = axis[a];
        DeviceAxis &d = dev[a];
        const size_t n_w = (size_t)t.dst * 8 * 4, n_first = (size_t)t.dst * 4, bytes = n_w + 2 * n_first;
        if (!d.is(t)) {
            d.dst = 0;
            if (bytes > d.capacity) {
                if (d.mem) (void)hipFree(d.mem);     // hipFree waits for the work that still reads the old table
                d.mem = nullptr;
                d.capacity = 0;
                BT_HIP(hipMalloc((void **)&d.mem, bytes));
                d.capacity = bytes;
            }
            BT_HIP(hipMemcpyAsync(d.mem, t.weights.data(), n_w, hipMemcpyHostToDevice, s));
            BT_HIP(hipMemcpyAsync(d.mem + n_w, t.first.data(), n_first, hipMemcpyHostToDevice, s));
            BT_HIP(hipMemcpyAsync(d.mem + n_w + n_first, t.nearest.data(), n_first, hipMemcpyHostToDevice, s));
            d.src = t.src;
            d.dst = t.dst;
            last_stream = s;
            in_flight = true;
        }
        out.weights = (const float *)d.mem;
        out.first = (const int32_t *)(d.mem + n_w);
        out.nearest = (const uint32_t *)(d.mem + n_w + n_first);
        return 0;
    }
};

namespace {

bool bad_frame(uint32_t w, uint32_t h) {
    return w == 0 || h == 0 || (uint64_t)w * h > 0xffffffffull || w > 0x7fffffffu || h > 0x7fffffffu;
}

const bt_upscale_guides kNoGuides = {nullptr, 0, nullptr, 0, nullptr, 0};

int check_args(const void *handle, const float *color, uint32_t samples, uint32_t w, uint32_t h, const bt_upscale_guides &lo,
               const bt_upscale_guides &hi, const float *out, uint32_t W, uint32_t H, const bt_upscale_params &p, bool with_handle) {
    // in the order the header gives
    if ((with_handle && !handle) || !color || !out) return fail(BT_ERR_INVALID_ARG, "null upscale handle, colour or output buffer");
    if (samples == 0) return fail(BT_ERR_INVALID_ARG, "colour frame with 0 samples");
    if (bad_frame(w, h) || bad_frame(W, H)) return fail(BT_ERR_INVALID_ARG, "zero-sized or too large a frame (input or output)");
    if (W < w || H < h)
        return fail(BT_ERR_INVALID_ARG, "the upscale stage does not reduce: " + std::to_string(w) + "x" + std::to_string(h) + " -> " +
                                            std::to_string(W) + "x" + std::to_string(H) + " is a case for bt_resample");
    const float *lo_p[3] = {lo.albedo, lo.normal, lo.depth}, *hi_p[3] = {hi.albedo, hi.normal, hi.depth};
    const uint32_t lo_n[3] = {lo.albedo_samples, lo.normal_samples, lo.depth_samples};
    const uint32_t hi_n[3] = {hi.albedo_samples, hi.normal_samples, hi.depth_samples};
    const char *names[3] = {"albedo", "normal", "depth"};
    if (out == color) return fail(BT_ERR_INVALID_ARG, "the output must not alias the colour frame: every tap is the input's");
    for (int g = 0; g < 3; ++g)
        if (out == lo_p[g] || out == hi_p[g]) return fail(BT_ERR_INVALID_ARG, std::string("the output must not alias the ") + names[g] + " guide");
    for (int g = 0; g < 3; ++g)
        if ((lo_p[g] != nullptr) != (hi_p[g] != nullptr))
            return fail(BT_ERR_INVALID_ARG, std::string("the ") + names[g] + " guide is given at one size only: a pair needs both");
    for (int g = 0; g < 3; ++g)
        if (lo_p[g] && (lo_n[g] == 0 || hi_n[g] == 0)) return fail(BT_ERR_INVALID_ARG, std::string("the ") + names[g] + " guide has 0 samples");
    if (!std::isfinite(p.sigma_depth) || !(p.sigma_depth > 0.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_upscale_params.sigma_depth must be finite and > 0");
    if (!std::isfinite(p.sigma_albedo) || !(p.sigma_albedo > 0.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_upscale_params.sigma_albedo must be finite and > 0");
    if (p.normal_squarings > 6u)
        return fail(BT_ERR_INVALID_ARG, "bt_upscale_params.normal_squarings " + std::to_string(p.normal_squarings) + " is outside 0 .. 6");
    if (!std::isfinite(p.min_weight) || !(p.min_weight > 0.0f) || !(p.min_weight < 1.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_upscale_params.min_weight must lie in (0, 1)");
    if (!std::isfinite(p.max_value) || !(p.max_value > 0.0f))
        return fail(BT_ERR_INVALID_ARG, "bt_upscale_params.max_value must be finite and > 0");
    return 0;
}

bt_upscale_params params_or_default(const bt_upscale_params *params) {
    bt_upscale_params p;
    if (params) p = *params;
    else bt_upscale_params_default(&p);
    return p;
}

btupscale::Weights weights_of(const bt_upscale_params &p) {
    btupscale::Weights P;
    P.sigma_depth = p.sigma_depth;
    P.k_a = 1.0f / (p.sigma_albedo * p.sigma_albedo);
    P.min_weight = p.min_weight;
    P.squarings = p.normal_squarings;
    return P;
}

float recip(uint32_t n) { return n ? 1.0f / (float)n : 0.0f; }

BtUpscaleGuides device_guides(const bt_upscale_guides &g) {
    return BtUpscaleGuides{g.albedo, g.normal, g.depth, recip(g.albedo_samples), recip(g.normal_samples), recip(g.depth_samples)};
}

btupscale::Guides host_guides(const bt_upscale_guides &g) {
    return btupscale::Guides{(const btupscale::Texel *)g.albedo, (const btupscale::Texel *)g.normal, (const btupscale::Texel *)g.depth,
                             recip(g.albedo_samples), recip(g.normal_samples), recip(g.depth_samples)};
}

} // namespace

extern "C" {

void bt_upscale_params_default(bt_upscale_params *out) {
    if (!out) return;
    // starting values (DESIGN.md 19 has the sweep around them); max_value is the glare and resample stages' cap
    out->sigma_depth = 0.1f;
    out->sigma_albedo = 0.1f;
    out->normal_squarings = 3;
    out->min_weight = 0.01f;
    out->max_value = 65536.0f;
}

bt_upscale *bt_upscale_new(void) { return new bt_upscale(); }

void bt_upscale_free(bt_upscale *h) { delete h; }

int bt_upscale_device(bt_upscale *h, const float *color_device, uint32_t color_samples, uint32_t width, uint32_t height,
                      const bt_upscale_guides *lo, const bt_upscale_guides *hi, float *out_device, uint32_t out_width, uint32_t out_height,
                      const bt_upscale_params *params, void *stream) {
    const bt_upscale_params p = params_or_default(params);
    const bt_upscale_guides &gl = lo ? *lo : kNoGuides, &gh = hi ? *hi : kNoGuides;
    int rc = check_args(h, color_device, color_samples, width, height, gl, gh, out_device, out_width, out_height, p, true);
    if (rc) return rc;
    rc = h->bind();                      // BT_ERR_DEVICE without a device, before any table is built
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    h->called = false;                   // until both launches have been enqueued
    if ((rc = h->table(0, width, out_width)) || (rc = h->table(1, height, out_height))) return rc;
    const size_t texels = (size_t)width * height;
    if (texels > h->capacity) {
        if (h->planes) (void)hipFree(h->planes);     // hipFree waits for the work that still reads the old planes
        h->planes = nullptr;
        h->capacity = 0;
        BT_HIP(hipMalloc((void **)&h->planes, texels * 3 * 16));
        h->capacity = texels;
    }
    if (!h->counters) BT_HIP(hipMalloc((void **)&h->counters, sizeof(unsigned long long)));
    BtUpscaleAxis ax, ay;
    if ((rc = h->upload(0, s, ax)) || (rc = h->upload(1, s, ay))) return rc;
    h->last_stream = s;
    h->in_flight = true;
    BT_HIP(hipMemsetAsync(h->counters, 0, sizeof(unsigned long long), s));
    BT_HIP(bt_launch_upscale_prepare(color_device, 1.0f / (float)color_samples, p.max_value, device_guides(gl), width, height, h->planes, s));
    BT_HIP(bt_launch_upscale(h->planes, color_device, width, height, device_guides(gh), out_device, out_width, out_height, ax, ay,
                             weights_of(p), h->counters, s));
    h->pw = width;
    h->ph = height;
    h->pixels = (uint32_t)((uint64_t)out_width * out_height);
    h->called = true;
    return 0;
}

int bt_upscale_poll(bt_upscale *h, bt_upscale_stats *out) {
    if (!h || !out) return fail(BT_ERR_INVALID_ARG, "null upscale handle or stats");
    if (!h->called || !h->counters) return fail(BT_ERR_INVALID_ARG, "bt_upscale_poll before a bt_upscale_device call");
    unsigned long long c = 0;
    BT_HIP(hipStreamSynchronize(h->last_stream));
    h->in_flight = false;
    BT_HIP(hipMemcpy(&c, h->counters, sizeof c, hipMemcpyDeviceToHost));
    out->tier2 = (uint32_t)(c & 0xffffffffull);
    out->tier3 = (uint32_t)(c >> 32);
    out->pixels = h->pixels;
    out->reserved = 0;
    return 0;
}

int bt_debug_upscale_weights(bt_upscale *h, int axis, uint32_t *sides, int32_t *first, float *weights, uint32_t *nearest) {
    if (!h) return fail(BT_ERR_INVALID_ARG, "null upscale handle");
    if (axis != 0 && axis != 1) return fail(BT_ERR_INVALID_ARG, "axis " + std::to_string(axis) + ": 0 is x, 1 is y");
    const btupscale::Axis &t = h->axis[axis];
    if (t.dst == 0) return fail(BT_ERR_INVALID_ARG, "the handle has no table yet: there has been no call");
    if (sides) {
        sides[0] = t.src;
        sides[1] = t.dst;
    }
    if (first) std::copy(t.first.begin(), t.first.end(), first);
    if (weights) std::copy(t.weights.begin(), t.weights.end(), weights);
    if (nearest) std::copy(t.nearest.begin(), t.nearest.end(), nearest);
    return 8;
}

int bt_debug_upscale_plane(bt_upscale *h, uint32_t which, float *host, uint32_t n) {
    if (!h) return fail(BT_ERR_INVALID_ARG, "null upscale handle");
    if (which > 2u) return fail(BT_ERR_INVALID_ARG, "plane " + std::to_string(which) + ": 0 is (colour, depth), 1 the normal, 2 the albedo");
    if (!h->called || !h->planes) return fail(BT_ERR_INVALID_ARG, "the handle has no planes: there has been no device call");
    const uint64_t count = (uint64_t)h->pw * h->ph * 4;
    if (count > 0x7fffffffull) return fail(BT_ERR_INVALID_ARG, "the plane has more elements than the return value can count");
    if (n == 0) return (int)count;
    if (!host) return fail(BT_ERR_INVALID_ARG, "null buffer");
    n = (uint32_t)std::min<uint64_t>(n, count);
    BT_HIP(hipStreamSynchronize(h->last_stream));
    h->in_flight = false;
    BT_HIP(hipMemcpy(host, h->planes + (size_t)which * count, (size_t)n * 4, hipMemcpyDeviceToHost));
    return (int)n;
}

int bt_debug_upscale_host(bt_upscale *h, const float *color_host, uint32_t color_samples, uint32_t width, uint32_t height,
                          const bt_upscale_guides *lo, const bt_upscale_guides *hi, float *out_host, uint32_t out_width, uint32_t out_height,
                          const bt_upscale_params *params, bt_upscale_stats *stats) {
    const bt_upscale_params p = params_or_default(params);
    const bt_upscale_guides &gl = lo ? *lo : kNoGuides, &gh = hi ? *hi : kNoGuides;
    int rc = check_args(nullptr, color_host, color_samples, width, height, gl, gh, out_host, out_width, out_height, p, false);
    if (rc) return rc;
    static_assert(sizeof(btupscale::Texel) == 16, "a texel is four floats");
    btupscale::Axis local[2];
    btupscale::Axis *ax = &local[0], *ay = &local[1];
    if (h) {                             // the handle keeps the tables, for bt_debug_upscale_weights and for the next call
        if ((rc = h->table(0, width, out_width)) || (rc = h->table(1, height, out_height))) return rc;
        ax = &h->axis[0];
        ay = &h->axis[1];
    } else {
        btupscale::build_axis(local[0], width, out_width);
        btupscale::build_axis(local[1], height, out_height);
    }
    std::unique_ptr<btupscale::Texel[]> planes(new btupscale::Texel[(size_t)width * height * 3]);
    uint64_t tier2 = 0, tier3 = 0;
    btupscale::run_host((const btupscale::Texel *)color_host, color_samples, width, height, host_guides(gl), host_guides(gh),
                        (btupscale::Texel *)out_host, out_width, out_height, *ax, *ay, weights_of(p), p.max_value, planes.get(), &tier2,
                        &tier3);
    if (stats) {
        stats->tier2 = (uint32_t)tier2;
        stats->tier3 = (uint32_t)tier3;
        stats->pixels = (uint32_t)((uint64_t)out_width * out_height);
        stats->reserved = 0;
    }
    return 0;
}

} // extern "C"
