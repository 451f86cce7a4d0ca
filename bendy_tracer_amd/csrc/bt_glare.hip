// bt_glare.hip -- EXTENSION, NOT IN THE REFERENCE: the kernels of the glare stage (bt_glare*): an energy-conserving
// bloom over a pyramid of float4 planes, applied to a frame of running sums in scene-linear light.
//
//   bt_glare_down0_kernel      sanitises the sums and decimates them in one pass: reads the frame, writes D_1 (no full-resolution
//                              copy of the sanitised frame exists);
//   bt_glare_down_kernel       D_k from D_{k-1};
//   bt_glare_up_kernel         A_k = D_k * w_k + up(A_{k+1}), in place: a texel reads itself and the coarser plane;
//   bt_glare_composite_kernel  re-reads the sums, re-forms s, takes the four A_1 taps, writes the mean `out`;
//   bt_glare_mean_kernel       L = 0: out = s.
// The direct form: one thread per output texel, 16 x 16 workgroups, every tap one 16-byte load at a clamped index.  The last
// down kernel of a call multiplies by w_L (A_L = D_L * w_L; the others multiply by 1, which is exact), so a call is 2 L launches.
// In the product build (bt_glare.hpp's BT_GLARE_DOWN0_LDS; 0 builds the direct form) down0 stages the 34 x 34 sanitised texels its
// 16 x 16 outputs take in LDS, so each is fetched and sanitised once instead of four times: the same operations per texel in
// the same order, and faster on a rendered 1080p frame.
// Every operation on a texel is bt_glare.hpp's, which tests/glare_ref.py restates in numpy.
#include <hip/hip_runtime.h>

#include <cstdint>

#define BT_GLARE_LAUNCHERS
#include "bt_glare.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr uint32_t kTile = 16;
#if BT_GLARE_DOWN0_LDS
constexpr uint32_t kStage = 2 * kTile + 2;      // the taps 2i-1 .. 2i+2 of 16 outputs on an axis
#endif

// the workgroup's tile from a one-dimensional grid (grid.y is limited to 65535, a frame's height is not)
__device__ inline bool texel_of(uint32_t tiles_x, uint32_t w, uint32_t h, uint32_t &x, uint32_t &y) {
    const uint32_t tile = blockIdx.x;
    x = (tile % tiles_x) * kTile + threadIdx.x;
    y = (tile / tiles_x) * kTile + threadIdx.y;
    return x < w && y < h;
}

} // namespace

__global__ __launch_bounds__(256) void bt_glare_down0_kernel(const float4 *__restrict__ sums, float r, float max_value, uint32_t sw,
                                                             uint32_t sh, float4 *__restrict__ dst, uint32_t dw, uint32_t dh,
                                                             uint32_t tiles_x, float w_out) {
    uint32_t i, j;
#if BT_GLARE_DOWN0_LDS
    __shared__ float4 stage[kStage * kStage];
    const bool inside = texel_of(tiles_x, dw, dh, i, j);
    // the tile's first taps (-1 for the first tile of an axis); entry (a, b) holds the texel at the clamped (ox + a, oy + b),
    // which is the texel every clamped tap x of this tile finds at a = x - ox
    const int64_t ox = 2 * (int64_t)((blockIdx.x % tiles_x) * kTile) - 1, oy = 2 * (int64_t)((blockIdx.x / tiles_x) * kTile) - 1;
    for (uint32_t e = threadIdx.y * kTile + threadIdx.x; e < kStage * kStage; e += kTile * kTile) {
        const int64_t px = ox + (int64_t)(e % kStage), py = oy + (int64_t)(e / kStage);
        const uint32_t x = px < 0 ? 0u : px > (int64_t)sw - 1 ? sw - 1u : (uint32_t)px;
        const uint32_t y = py < 0 ? 0u : py > (int64_t)sh - 1 ? sh - 1u : (uint32_t)py;
        stage[e] = btglare::sanitise(sums[(size_t)y * sw + x], r, max_value);
    }
    __syncthreads();
    if (!inside) return;
    const float4 d = btglare::down_texel<float4>(
        [&](uint32_t x, uint32_t y) { return stage[(uint32_t)((int64_t)y - oy) * kStage + (uint32_t)((int64_t)x - ox)]; }, i, j, sw, sh);
#else
    if (!texel_of(tiles_x, dw, dh, i, j)) return;
    const float4 d = btglare::down_texel<float4>(
        [&](uint32_t x, uint32_t y) { return btglare::sanitise(sums[(size_t)y * sw + x], r, max_value); }, i, j, sw, sh);
#endif
    dst[(size_t)j * dw + i] = btglare::scale(d, w_out);
}

__global__ __launch_bounds__(256) void bt_glare_down_kernel(const float4 *__restrict__ src, uint32_t sw, uint32_t sh,
                                                            float4 *__restrict__ dst, uint32_t dw, uint32_t dh, uint32_t tiles_x,
                                                            float w_out) {
    uint32_t i, j;
    if (!texel_of(tiles_x, dw, dh, i, j)) return;
    const float4 d = btglare::down_texel<float4>([&](uint32_t x, uint32_t y) { return src[(size_t)y * sw + x]; }, i, j, sw, sh);
    dst[(size_t)j * dw + i] = btglare::scale(d, w_out);
}

__global__ __launch_bounds__(256) void bt_glare_up_kernel(float4 *__restrict__ plane, uint32_t w, uint32_t h,
                                                          const float4 *__restrict__ coarse, uint32_t cw, uint32_t ch, uint32_t tiles_x,
                                                          float w_k) {
    uint32_t x, y;
    if (!texel_of(tiles_x, w, h, x, y)) return;
    const float4 u = btglare::up_texel<float4>([&](uint32_t a, uint32_t b) { return coarse[(size_t)b * cw + a]; }, x, y, cw, ch);
    const size_t at = (size_t)y * w + x;
    plane[at] = btglare::accumulate(plane[at], w_k, u);
}

__global__ __launch_bounds__(256) void bt_glare_composite_kernel(const float4 *__restrict__ sums, float r, float max_value,
                                                                 float strength, const float4 *__restrict__ a1, uint32_t cw, uint32_t ch,
                                                                 float4 *__restrict__ out, uint32_t w, uint32_t h, uint32_t tiles_x) {
    uint32_t x, y;
    if (!texel_of(tiles_x, w, h, x, y)) return;
    const size_t at = (size_t)y * w + x;
    const float4 in = sums[at];
    const float4 g = btglare::up_texel<float4>([&](uint32_t a, uint32_t b) { return a1[(size_t)b * cw + a]; }, x, y, cw, ch);
    out[at] = btglare::composite(btglare::sanitise(in, r, max_value), g, strength, in.w);
}

__global__ __launch_bounds__(256) void bt_glare_mean_kernel(const float4 *__restrict__ sums, float r, float max_value,
                                                            float4 *__restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 in = sums[i];
    float4 s = btglare::sanitise(in, r, max_value);
    s.w = in.w;
    out[i] = s;
}

// ---- host-side launchers (called from bt_glare_api.cpp, which declares them too) ---------------------------
namespace {

// tiles of a w x h plane; false where the grid would not fit one launch
bool tiles_of(uint32_t w, uint32_t h, uint32_t &tiles_x, uint32_t &grid) {
    const uint64_t tx = ((uint64_t)w + kTile - 1) / kTile, ty = ((uint64_t)h + kTile - 1) / kTile;
    if (tx * ty * 256 > 0xffffffffull) return false;           // the runtime takes at most 2^32 - 1 threads per launch
    tiles_x = (uint32_t)tx;
    grid = (uint32_t)(tx * ty);
    return true;
}

} // namespace

extern "C" hipError_t bt_launch_glare_down0(const float *sums, uint32_t samples, float max_value, uint32_t sw, uint32_t sh, float *dst,
                                            uint32_t dw, uint32_t dh, float w_out, hipStream_t stream) {
    uint32_t tx, grid;
    if (!tiles_of(dw, dh, tx, grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(bt_glare_down0_kernel, dim3(grid), dim3(kTile, kTile), 0, stream, (const float4 *)sums, 1.0f / (float)samples,
                       max_value, sw, sh, (float4 *)dst, dw, dh, tx, w_out);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_glare_down(const float *src, uint32_t sw, uint32_t sh, float *dst, uint32_t dw, uint32_t dh, float w_out,
                                           hipStream_t stream) {
    uint32_t tx, grid;
    if (!tiles_of(dw, dh, tx, grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(bt_glare_down_kernel, dim3(grid), dim3(kTile, kTile), 0, stream, (const float4 *)src, sw, sh, (float4 *)dst, dw, dh,
                       tx, w_out);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_glare_up(float *plane, uint32_t w, uint32_t h, const float *coarse, uint32_t cw, uint32_t ch, float w_k,
                                         hipStream_t stream) {
    uint32_t tx, grid;
    if (!tiles_of(w, h, tx, grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(bt_glare_up_kernel, dim3(grid), dim3(kTile, kTile), 0, stream, (float4 *)plane, w, h, (const float4 *)coarse, cw,
                       ch, tx, w_k);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_glare_composite(const float *sums, uint32_t samples, float max_value, float strength, const float *a1,
                                                uint32_t cw, uint32_t ch, float *out, uint32_t w, uint32_t h, hipStream_t stream) {
    uint32_t tx, grid;
    if (!tiles_of(w, h, tx, grid)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(bt_glare_composite_kernel, dim3(grid), dim3(kTile, kTile), 0, stream, (const float4 *)sums,
                       1.0f / (float)samples, max_value, strength, (const float4 *)a1, cw, ch, (float4 *)out, w, h, tx);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_glare_mean(const float *sums, uint32_t samples, float max_value, float *out, uint64_t n,
                                           hipStream_t stream) {
    if ((n + 255) / 256 * 256 > 0xffffffffull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(bt_glare_mean_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, (const float4 *)sums,
                       1.0f / (float)samples, max_value, (float4 *)out, n);
    return hipGetLastError();
}
