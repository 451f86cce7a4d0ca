// bt_display.hip -- EXTENSION, NOT IN THE REFERENCE: the kernels of the display stage (bt_display*): metered
// auto-exposure and tone mapping of a frame of running sums into RGBA8.
//
//   bt_meter_kernel   a histogram of the frame's luminance: 256 bins of an eighth of an octave over [2^-16, 2^16) plus the
//                     counters `under` and `over`, built per workgroup in LDS and added to the handle's live counters;
//   bt_expose_kernel  one workgroup, one thread per bin: the mean of the bin centres between two percentiles, the exposure
//                     that brings it to the key, the adaptation towards it, mult = exp2_bt(e); it keeps a copy of the
//                     counters for bt_debug_display_histogram and clears the live ones for the next call;
//   bt_show_kernel    bt_preview_kernel with `* mult` and a tone operator between the mean and the colour space.
// All three run on the caller's stream; the exposure never visits the host.  The counts are integers, so no result depends on
// the order in which pixels are counted.  The order of every float32 operation and the Makefile's -ffp-contract=off are
// what tests/display_ref.py restates in numpy.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bt_color.hpp"
#include "bt_internal.hpp"

#pragma STDC FP_CONTRACT OFF

// A/B build (-DBT_METER_MERGE=1): lanes of a wave that count into the same bin elect one of them to add their number, instead
// of each adding 1 (DESIGN.md 15 has both forms' times).  Not the product build.
#ifndef BT_METER_MERGE
#define BT_METER_MERGE 0
#endif

namespace {

#ifndef BT_METER_UNROLL
#define BT_METER_UNROLL 4
#endif
#ifndef BT_METER_MAX_GRID
#define BT_METER_MAX_GRID 1024
#endif
#ifndef BT_METER_GROUP_PIXELS
#define BT_METER_GROUP_PIXELS 2048
#endif
constexpr int kMeterUnroll = BT_METER_UNROLL;                       // pixels a lane has in flight
constexpr uint32_t kMeterMaxGrid = BT_METER_MAX_GRID;               // larger frames take more strides
constexpr uint32_t kMeterPixelsPerGroup = BT_METER_GROUP_PIXELS;    // a workgroup's share of a frame that needs fewer workgroups

BT_DEV uint32_t meter_bin(float4 s, float r) {
    const float cx = s.x * r, cy = s.y * r, cz = s.z * r;                   // bt_preview_kernel's mean
    const float Y = (0.2126f * cx + 0.7152f * cy) + 0.0722f * cz;           // the luminance of DESIGN.md 13
    if (!(Y >= 0x1p-16f)) return BT_DISPLAY_BINS;                            // under: zero, negatives, NaN
    if (Y >= 0x1p16f) return BT_DISPLAY_BINS + 1;                            // over: +inf too
    return (__float_as_uint(Y) >> 20) - 888u;                               // exponent and three mantissa bits: 0 .. 255
}

BT_DEV void meter_count(uint32_t *h, uint32_t bin) {
#if BT_METER_MERGE
    for (;;) {
        const uint32_t lead = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
        const unsigned long long same = __ballot(bin == lead);
        if (bin == lead) {
            if ((unsigned)__lane_id() == (unsigned)__ffsll((long long)same) - 1u) atomicAdd(&h[lead], (uint32_t)__popcll(same));
            break;
        }
    }
#else
    atomicAdd(&h[bin], 1u);
#endif
}

template <int OP>
BT_DEV float tone(float x, float iw2) {
    if (OP == BT_TONEMAP_CLIP) return x;
    x = x > 0.0f ? x : 0.0f;
    if (OP == BT_TONEMAP_REINHARD) return (x * (1.0f + x * iw2)) / (1.0f + x);
    return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);   // Narkowicz's fit of the ACES curve
}

} // namespace

__global__ __launch_bounds__(256) void bt_meter_kernel(const float4 *rgba, uint64_t n, float samples_recip, uint32_t *live) {
    __shared__ uint32_t h[BT_DISPLAY_STRIDE];
    const uint32_t tid = threadIdx.x;
    h[tid] = 0;
    if (tid < BT_DISPLAY_STRIDE - 256) h[256 + tid] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + tid; i < n; i += stride * kMeterUnroll) {
        float4 s[kMeterUnroll];
#pragma unroll
        for (int k = 0; k < kMeterUnroll; ++k) {
            const uint64_t j = i + stride * k;
            if (j < n) s[k] = rgba[j];
        }
#pragma unroll
        for (int k = 0; k < kMeterUnroll; ++k)
            if (i + stride * k < n) meter_count(h, meter_bin(s[k], samples_recip));
    }
    __syncthreads();
    for (uint32_t b = tid; b < BT_DISPLAY_COUNTERS; b += 256) {
        const uint32_t v = h[b];
        if (v) atomicAdd(&live[b], v);
    }
}

__global__ __launch_bounds__(256) void bt_expose_kernel(uint32_t *live, uint32_t *last, BtDisplayState *state, BtDisplayExpose p) {
    __shared__ uint32_t incl[BT_DISPLAY_BINS];
    __shared__ unsigned long long sw[BT_DISPLAY_BINS], ss[BT_DISPLAY_BINS];
    const uint32_t b = threadIdx.x;
    const uint32_t hb = live[b];
    last[b] = hb;
    live[b] = 0;
    if (b < BT_DISPLAY_COUNTERS - BT_DISPLAY_BINS) {
        last[BT_DISPLAY_BINS + b] = live[BT_DISPLAY_BINS + b];
        live[BT_DISPLAY_BINS + b] = 0;
    }
    // inclusive prefix sum of the counts (N <= the frame's pixels < 2^32)
    incl[b] = hb;
    __syncthreads();
    for (uint32_t d = 1; d < BT_DISPLAY_BINS; d <<= 1) {
        const uint32_t v = b >= d ? incl[b - d] : 0u;
        __syncthreads();
        incl[b] += v;
        __syncthreads();
    }
    const uint64_t N = incl[BT_DISPLAY_BINS - 1];
    const uint64_t lo = (uint64_t)__builtin_floor((double)p.p_low * (double)N);
    const uint64_t hi = N - (uint64_t)__builtin_floor((double)p.p_high * (double)N);
    const uint64_t P1 = incl[b], P0 = P1 - hb;
    const uint64_t top = P1 < hi ? P1 : hi, bot = P0 > lo ? P0 : lo;
    const uint64_t w = top > bot ? top - bot : 0;          // the bin's pixels between the two percentiles
    sw[b] = w;
    ss[b] = w * (2 * b + 1);
    __syncthreads();
    for (uint32_t d = BT_DISPLAY_BINS / 2; d > 0; d >>= 1) {
        if (b < d) {
            sw[b] += sw[b + d];
            ss[b] += ss[b + d];
        }
        __syncthreads();
    }
    if (b != 0) return;
    const uint64_t W = sw[0], S = ss[0];
    float e = state->e;
    uint32_t valid = state->valid;
    if (W != 0) {
        const double m = (double)S / (16.0 * (double)W) - 16.0;       // the mean of the bin centres in log2
        float t = (float)(p.log2_key - m) + p.ev;
        t = t < p.ev_min ? p.ev_min : t;
        t = t > p.ev_max ? p.ev_max : t;
        if (!valid || p.adapt >= 1.0f) e = t;
        else e = e + (t - e) * p.adapt;
        valid = 1;
        state->e = e;
        state->valid = valid;
    }
    const float shown = valid ? e : p.ev;                   // a black frame: the state is left alone
    state->shown_ev = shown;
    state->shown_mult = exp2_bt(shown);
}

template <int OP>
__global__ __launch_bounds__(256) void bt_show_kernel(const float4 *rgba, uint32_t *out, uint64_t n, float samples_recip,
                                                      int color_space, float iw2, int manual, float ev, BtDisplayState *state) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const float mult = manual ? exp2_bt(ev) : state->shown_mult;       // wave-uniform either way
    if (manual && i == 0) {                                 // for bt_display_exposure; (e, valid) stay as they are
        state->shown_ev = ev;
        state->shown_mult = mult;
    }
    if (i >= n) return;
    const float4 s = rgba[i];
    float x = tone<OP>((s.x * samples_recip) * mult, iw2);
    float y = tone<OP>((s.y * samples_recip) * mult, iw2);
    float z = tone<OP>((s.z * samples_recip) * mult, iw2);
    if (color_space == BT_COLOR_SRGB) {
        x = linear_to_srgb(x);
        y = linear_to_srgb(y);
        z = linear_to_srgb(z);
    }
    out[i] = f32_to_u8(x) | (f32_to_u8(y) << 8) | (f32_to_u8(z) << 16) | (f32_to_u8(s.w) << 24);
}

// ---- host-side launchers (called from bt_display_api.cpp) ------------------------------------------------
extern "C" hipError_t bt_launch_display_meter(const float *rgba, uint64_t n, uint32_t samples, uint32_t *live, hipStream_t stream) {
    const uint64_t groups = (n + kMeterPixelsPerGroup - 1) / kMeterPixelsPerGroup;
    const uint32_t grid = (uint32_t)(groups < kMeterMaxGrid ? groups : kMeterMaxGrid);
    hipLaunchKernelGGL(bt_meter_kernel, dim3(grid), dim3(256), 0, stream, (const float4 *)rgba, n, 1.0f / (float)samples, live);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_display_expose(uint32_t *live, uint32_t *last, BtDisplayState *state, const BtDisplayExpose *p,
                                               hipStream_t stream) {
    hipLaunchKernelGGL(bt_expose_kernel, dim3(1), dim3(BT_DISPLAY_BINS), 0, stream, live, last, state, *p);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_display_show(const float *rgba, uint8_t *out, uint64_t n, uint32_t samples, int color_space, int op,
                                             float iw2, int manual, float ev, BtDisplayState *state, hipStream_t stream) {
    const dim3 grid((uint32_t)((n + 255) / 256)), block(256);
    const float recip = 1.0f / (float)samples;
    if (op == BT_TONEMAP_CLIP)
        hipLaunchKernelGGL(bt_show_kernel<BT_TONEMAP_CLIP>, grid, block, 0, stream, (const float4 *)rgba, (uint32_t *)out, n, recip,
                           color_space, iw2, manual, ev, state);
    else if (op == BT_TONEMAP_REINHARD)
        hipLaunchKernelGGL(bt_show_kernel<BT_TONEMAP_REINHARD>, grid, block, 0, stream, (const float4 *)rgba, (uint32_t *)out, n,
                           recip, color_space, iw2, manual, ev, state);
    else
        hipLaunchKernelGGL(bt_show_kernel<BT_TONEMAP_ACES>, grid, block, 0, stream, (const float4 *)rgba, (uint32_t *)out, n, recip,
                           color_space, iw2, manual, ev, state);
    return hipGetLastError();
}
