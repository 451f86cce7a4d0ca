// bt_resample.hip -- EXTENSION, NOT IN THE REFERENCE: the kernels of the resample stage (bt_resample*): a separable
// filter from a frame of w x h running sums to a W x H mean, in scene-linear light.
//
//   bt_resample_h_kernel   reads the sums, sanitises them and filters along x into the plane P (W x h); a full-size sanitised copy
//                          never exists;
//   bt_resample_v_kernel   filters P along y, clamps, fetches the alpha of the nearest input pixel and writes the mean (W x H).
// One thread per output texel, workgroups of 32 x 8 outputs on a one-dimensional grid, every tap one 16-byte load at an index
// that is clamped first.  The first pass has two forms (template argument), bit-identical because both run bt_resample.hpp's
// filter_texel over the same texels in the same order:
//   staged   the workgroup's outputs take a contiguous span of the source row (the table's first taps never decrease), which is
//            loaded and sanitised once into LDS: 8 rows of up to 192 texels;
//   direct   every tap is a clamped global load and a sanitise.
// The launcher takes the staged form where a row has 6 taps and more and the pass's widest span fits (bt_resample.hpp:
// BT_RESAMPLE_STAGE_MIN_TAPS, BT_RESAMPLE_STAGE_X) and the direct form elsewhere: with fewer taps the direct form is faster
// (DESIGN.md 17 has the times); -DBT_RESAMPLE_LDS=0 builds the direct form alone.  The second pass is direct: its taps run down a
// column, so a wave's loads are whole rows of 512 B already, and a staged form of it was slower in five cases of six and was
// removed.  Weights, first taps and nearest indices come from the handle's tables through ordinary vector loads.
#include <hip/hip_runtime.h>

#include <cstdint>

#define BT_RESAMPLE_LAUNCHERS
#include "bt_resample.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr uint32_t kTX = BT_RESAMPLE_TILE_X, kTY = BT_RESAMPLE_TILE_Y;
[[maybe_unused]] constexpr uint32_t kStageX = BT_RESAMPLE_STAGE_X;

// the first and the last source texel that the outputs i0 .. i0 + n - 1 (cut at `dst`) take, taps clamped to `side`
[[maybe_unused]] __device__ inline void tile_span(const int32_t *first, uint32_t taps, uint32_t i0, uint32_t n, uint32_t dst, uint32_t side,
                                 uint32_t &origin, uint32_t &end) {
    const uint32_t i1 = i0 + n < dst ? i0 + n - 1 : dst - 1;
    origin = btresample::clamp_index(first[i0], side);
    end = btresample::clamp_index((int64_t)first[i1] + taps - 1, side);
}

} // namespace

template <bool kStaged>
__global__ __launch_bounds__(256) void bt_resample_h_kernel(const float4 *__restrict__ sums, float r, float max_value, uint32_t w,
                                                            uint32_t h, float4 *__restrict__ plane, uint32_t W,
                                                            const int32_t *__restrict__ first, const float *__restrict__ weights,
                                                            uint32_t taps, uint32_t tiles_x) {
    const uint32_t i0 = (blockIdx.x % tiles_x) * kTX, i = i0 + threadIdx.x, y = (blockIdx.x / tiles_x) * kTY + threadIdx.y;
    const bool inside = i < W && y < h;
    if constexpr (kStaged) {
        __shared__ float4 stage[kTY * kStageX];
        uint32_t origin, end;
        tile_span(first, taps, i0, kTX, W, w, origin, end);
        // the launcher has checked that no tile's span exceeds kStageX; the bound below keeps a stray table inside the array
        const uint32_t span = end - origin + 1 < kStageX ? end - origin + 1 : kStageX;
        float4 *mine = stage + threadIdx.y * kStageX;
        if (y < h)
            for (uint32_t c = threadIdx.x; c < span; c += kTX) mine[c] = btglare::sanitise(sums[(size_t)y * w + origin + c], r, max_value);
        __syncthreads();
        if (!inside) return;
        plane[(size_t)y * W + i] = btresample::filter_texel<float4>(
            [&](uint32_t p) {
                const uint32_t c = p - origin;
                return mine[c < kStageX ? c : kStageX - 1];
            },
            weights + (size_t)i * taps, first[i], taps, w);
    } else {
        if (!inside) return;
        const float4 *row = sums + (size_t)y * w;
        plane[(size_t)y * W + i] = btresample::filter_texel<float4>([&](uint32_t p) { return btglare::sanitise(row[p], r, max_value); },
                                                                     weights + (size_t)i * taps, first[i], taps, w);
    }
}

__global__ __launch_bounds__(256) void bt_resample_v_kernel(const float4 *__restrict__ plane, uint32_t W, uint32_t h,
                                                            float4 *__restrict__ out, uint32_t H, const int32_t *__restrict__ first,
                                                            const float *__restrict__ weights, uint32_t taps,
                                                            const uint32_t *__restrict__ nearest_x, const uint32_t *__restrict__ nearest_y,
                                                            const float4 *__restrict__ sums, uint32_t w, int clamp_negative,
                                                            uint32_t tiles_x) {
    const uint32_t i = (blockIdx.x % tiles_x) * kTX + threadIdx.x, j = (blockIdx.x / tiles_x) * kTY + threadIdx.y;
    if (i >= W || j >= H) return;
    const float4 acc = btresample::filter_texel<float4>([&](uint32_t p) { return plane[(size_t)p * W + i]; }, weights + (size_t)j * taps,
                                                        first[j], taps, h);
    out[(size_t)j * W + i] = btresample::finish(acc, clamp_negative, sums[(size_t)nearest_y[j] * w + nearest_x[i]].w);
}

// ---- host-side launchers (called from bt_resample_api.cpp, which declares them too) ------------------------
namespace {

// tiles of a plane of `cols` x `rows` outputs; false where the grid would not fit one launch
bool tiles_of(uint32_t cols, uint32_t rows, uint32_t &tiles_x, uint32_t &grid) {
    const uint64_t tx = ((uint64_t)cols + kTX - 1) / kTX, ty = ((uint64_t)rows + kTY - 1) / kTY;
    if (tx * ty * 256 > 0xffffffffull) return false;           // the runtime takes at most 2^32 - 1 threads per launch
    tiles_x = (uint32_t)tx;
    grid = (uint32_t)(tx * ty);
    return true;
}

} // namespace

extern "C" hipError_t bt_launch_resample_h(const float *sums, uint32_t samples, float max_value, uint32_t w, uint32_t h, float *plane,
                                           uint32_t W, BtResampleAxis ax, hipStream_t stream) {
    uint32_t tx, grid;
    if (!tiles_of(W, h, tx, grid)) return hipErrorInvalidConfiguration;
    const float r = 1.0f / (float)samples;
#if BT_RESAMPLE_LDS
    if (ax.taps >= BT_RESAMPLE_STAGE_MIN_TAPS && ax.widest <= kStageX)
        hipLaunchKernelGGL(bt_resample_h_kernel<true>, dim3(grid), dim3(kTX, kTY), 0, stream, (const float4 *)sums, r, max_value, w, h,
                           (float4 *)plane, W, ax.first, ax.weights, ax.taps, tx);
    else
#endif
        hipLaunchKernelGGL(bt_resample_h_kernel<false>, dim3(grid), dim3(kTX, kTY), 0, stream, (const float4 *)sums, r, max_value, w, h,
                           (float4 *)plane, W, ax.first, ax.weights, ax.taps, tx);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_resample_v(const float *plane, uint32_t W, uint32_t h, float *out, uint32_t H, BtResampleAxis ay,
                                           const uint32_t *nearest_x, const float *sums, uint32_t w, int clamp_negative,
                                           hipStream_t stream) {
    uint32_t tx, grid;
    if (!tiles_of(W, H, tx, grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(bt_resample_v_kernel, dim3(grid), dim3(kTX, kTY), 0, stream, (const float4 *)plane, W, h, (float4 *)out, H, ay.first,
                       ay.weights, ay.taps, nearest_x, ay.nearest, (const float4 *)sums, w, clamp_negative, tx);
    return hipGetLastError();
}
