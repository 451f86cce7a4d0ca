// bt_despeckle.hip -- EXTENSION, NOT IN THE REFERENCE: the kernel of the despeckle stage (bt_despeckle*): rank-order
// firefly rejection on a frame of running sums, ahead of every other stage.
//
// One launch per call: 16 x 16 workgroups on a one-dimensional grid of tiles, one thread per pixel, templated on the radius.  A
// thread keeps its own sanitised float4 in registers.  In the product build (bt_despeckle.hpp's BT_DESPECKLE_LDS; 0 builds the
// direct form) the workgroup stages the (16 + 2 R)^2 luminances of its tile and halo in LDS -- every thread its own pixel's, the
// first 68 or 144 threads one halo texel each, so a texel is fetched, sanitised and weighed once per tile instead of 9 or 25
// times -- and every thread selects from that stage.  Absent taps hold -1; no address outside the frame is formed.  The two
// counters take one 64-bit atomic per workgroup (none where it has nothing to add), after a ballot within each wave.
// Every operation on a pixel is bt_despeckle.hpp's, which tests/despeckle_ref.py restates in numpy.
#include <hip/hip_runtime.h>

#include <cstdint>

#define BT_DESPECKLE_LAUNCHERS
#include "bt_despeckle.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr uint32_t kTile = 16;

// entry `e` of the halo of a tile staged with side S = 16 + 2 R -> its column and row in the stage: the R rows above, the R rows
// below, then the R columns either side of each of the 16 rows between
template <int R>
__device__ inline void halo_entry(uint32_t e, uint32_t &a, uint32_t &b) {
    constexpr uint32_t S = kTile + 2 * R;
    if (e < R * S) {
        a = e % S;
        b = e / S;
    } else if (e < 2 * R * S) {
        a = (e - R * S) % S;
        b = kTile + R + (e - R * S) / S;
    } else {
        const uint32_t c = (e - 2 * R * S) % (2 * R);
        a = c < R ? c : kTile + c;
        b = R + (e - 2 * R * S) / (2 * R);
    }
}

} // namespace

template <int R>
__global__ __launch_bounds__(256) void bt_despeckle_kernel(const float4 *__restrict__ sums, float4 *__restrict__ out, uint32_t w, uint32_t h,
                                                           uint32_t tiles_x, uint32_t rank, float ratio, float fl, float cap,
                                                           unsigned long long *__restrict__ counters) {
    __shared__ uint32_t wave_counts[2 * 8];           // four waves of 64 lanes; room for eight of 32
    const uint32_t x0 = (blockIdx.x % tiles_x) * kTile, y0 = (blockIdx.x / tiles_x) * kTile;
    const uint32_t x = x0 + threadIdx.x, y = y0 + threadIdx.y, t = threadIdx.y * kTile + threadIdx.x;
    const bool inside = x < w && y < h;

    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool changed = false, flagged = false;
    float Y = -1.0f;
    if (inside) {
        s = btdespeckle::sanitise(sums[(size_t)y * w + x], cap, changed);
        Y = btdespeckle::luminance(s);
    }
#if BT_DESPECKLE_LDS
    constexpr uint32_t S = kTile + 2 * R;
    __shared__ float stage[S * S];
    stage[(threadIdx.y + R) * S + threadIdx.x + R] = Y;                 // -1 outside the frame
    if (t < S * S - kTile * kTile) {
        uint32_t a, b;
        halo_entry<R>(t, a, b);
        const int64_t px = (int64_t)x0 + a - R, py = (int64_t)y0 + b - R;
        float v = -1.0f;
        if (px >= 0 && py >= 0 && px < (int64_t)w && py < (int64_t)h) v = btdespeckle::weigh(sums[(size_t)py * w + (size_t)px], cap);
        stage[b * S + a] = v;
    }
    __syncthreads();
    const float *centre = stage + (threadIdx.y + R) * S + threadIdx.x + R;
    auto tap = [&](int i) {
        int dx, dy;
        btdespeckle::tap_offset<R>(i, dx, dy);
        return centre[dy * (int)S + dx];
    };
#else
    auto tap = [&](int i) {
        int dx, dy;
        btdespeckle::tap_offset<R>(i, dx, dy);
        const int64_t px = (int64_t)x + dx, py = (int64_t)y + dy;
        if (px < 0 || py < 0 || px >= (int64_t)w || py >= (int64_t)h) return -1.0f;
        return btdespeckle::weigh(sums[(size_t)py * w + (size_t)px], cap);
    };
#endif
    if (inside) {
        const uint32_t M = btdespeckle::neighbours(x, y, (uint32_t)R, w, h), k = rank < M ? rank : M;
        float lim = 0.0f;
        if (M > 0u) lim = btdespeckle::limit(btdespeckle::kth_largest<R>(tap, rank, k), ratio, fl);
        out[(size_t)y * w + x] = btdespeckle::apply(s, Y, lim, M, flagged);
    }
    // the counters: a ballot per wave, one atomic per workgroup
    const uint32_t n_flagged = (uint32_t)__popcll(__ballot(flagged)), n_changed = (uint32_t)__popcll(__ballot(changed));
    const uint32_t wave = t / warpSize, waves = kTile * kTile / warpSize;
    if (t % warpSize == 0) {
        wave_counts[2 * wave] = n_flagged;
        wave_counts[2 * wave + 1] = n_changed;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t f = 0, c = 0;
        for (uint32_t i = 0; i < waves; ++i) {
            f += wave_counts[2 * i];
            c += wave_counts[2 * i + 1];
        }
        // flagged in the low word, sanitised in the high one: neither can exceed the pixel count, which is below 2^32
        if (f | c) atomicAdd(counters, (unsigned long long)f | ((unsigned long long)c << 32));
    }
}

// ---- host-side launcher (called from bt_despeckle_api.cpp, which declares it too) ---------------------------
extern "C" hipError_t bt_launch_despeckle(const float *rgba, float *out, uint32_t width, uint32_t height, uint32_t radius, uint32_t rank,
                                          float ratio, float fl, float cap, uint32_t *counters, hipStream_t stream) {
    const uint64_t tx = ((uint64_t)width + kTile - 1) / kTile, ty = ((uint64_t)height + kTile - 1) / kTile;
    if (tx * ty * 256 > 0xffffffffull) return hipErrorInvalidConfiguration;        // the runtime takes at most 2^32 - 1 threads per launch
    const dim3 grid((uint32_t)(tx * ty)), block(kTile, kTile);
    if (radius == 1u)
        hipLaunchKernelGGL(bt_despeckle_kernel<1>, grid, block, 0, stream, (const float4 *)rgba, (float4 *)out, width, height, (uint32_t)tx, rank,
                           ratio, fl, cap, (unsigned long long *)counters);
    else if (radius == 2u)
        hipLaunchKernelGGL(bt_despeckle_kernel<2>, grid, block, 0, stream, (const float4 *)rgba, (float4 *)out, width, height, (uint32_t)tx, rank,
                           ratio, fl, cap, (unsigned long long *)counters);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}
