// bt_adapt.hip -- EXTENSION, NOT IN THE REFERENCE: the two small kernels of variance-driven adaptive sampling.
// The OUTPUT == 5 builds of bt_render_kernel (bt_kernels.hip) add a pass's samples to the tiles that are still active and keep
// each pixel's running sum of squared luminance; bt_adapt_update_kernel turns sums and moments into one error estimate per
// 16x16 tile and decides which tiles go on, bt_adapt_resolve_kernel divides every pixel by its own tile's sample count.
// Compiled with -ffp-contract=off like everything else: the operations below are the ones tests/adaptive_ref.py restates.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/bendy_hip.h"
#include "bt_internal.hpp"

namespace {
constexpr uint32_t TILE = BT_TILE;
}

// One workgroup of 256 threads per tile, one thread per pixel; runs behind the render kernel of the pass on its stream.
// T = samples per pixel the pass added to every active tile.
__global__ __launch_bounds__(256) void bt_adapt_update_kernel(const float4 *rgba, const float *moment, uint32_t *count,
                                                              uint32_t *active, float *error, uint32_t *n_active,
                                                              uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t T,
                                                              float threshold, uint32_t min_samples, uint32_t max_samples,
                                                              float eps) {
    __shared__ float s_part[4];
    const uint32_t tile = blockIdx.x;
    if (active[tile] == 0u) return;                    // wave-uniform: a tile that has stopped is never looked at again
    const uint32_t c = count[tile] + T;                // (every thread reads it ahead of the barrier, thread 0 writes behind it)
    const uint32_t tx = tile % tiles_x, ty = tile / tiles_x;
    const uint32_t px = tx * TILE + (threadIdx.x & 15u), py = ty * TILE + (threadIdx.x >> 4);
    float e = 0.0f;
    if (px < width && py < height) {
        const size_t i = (size_t)py * width + px;
        const float4 s = rgba[i];
        const float M = moment[i], cf = (float)c;
        const float S = (0.2126f * s.x + 0.7152f * s.y) + 0.0722f * s.z;
        const float mu = S / cf;
        const float var = fmaxf(0.0f, M / cf - mu * mu);
        const float ep = __builtin_sqrtf(var / cf) / (mu + eps);
        e = __builtin_isfinite(ep) ? ep : 0.0f;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off, 64);
    if ((threadIdx.x & 63u) == 0u) s_part[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t nx = width - tx * TILE < TILE ? width - tx * TILE : TILE;
        const uint32_t ny = height - ty * TILE < TILE ? height - ty * TILE : TILE;
        const float e_t = ((s_part[0] + s_part[1]) + (s_part[2] + s_part[3])) / (float)(nx * ny);
        const bool go_on = !(c >= max_samples || (c >= min_samples && e_t <= threshold));
        count[tile] = c;
        error[tile] = e_t;
        active[tile] = go_on ? 1u : 0u;
        if (go_on) atomicAdd(n_active, 1u);
    }
}

// out.rgb = sum.rgb * (1 / count of the pixel's tile) -- bt_preview_kernel's first line with the tile's own count --, out.a =
// sum.a; a tile without samples gives 0.
__global__ __launch_bounds__(256) void bt_adapt_resolve_kernel(const float4 *rgba, const uint32_t *count, float4 *out,
                                                               uint32_t width, uint32_t height, uint32_t tiles_x) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width * height) return;
    const uint32_t py = i / width, px = i - py * width;
    const uint32_t c = count[(py / TILE) * tiles_x + px / TILE];
    const float4 s = rgba[i];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, s.w);
    if (c != 0u) {
        const float recip = 1.0f / (float)c;
        o.x = s.x * recip;
        o.y = s.y * recip;
        o.z = s.z * recip;
    }
    out[i] = o;
}

extern "C" hipError_t bt_launch_adapt_update(const float *rgba, const float *moment, uint32_t *count, uint32_t *active,
                                             float *error, uint32_t *n_active, uint32_t width, uint32_t height, uint32_t T,
                                             const bt_adaptive_params *p, hipStream_t stream) {
    const uint32_t tiles_x = (width + TILE - 1) / TILE, tiles_y = (height + TILE - 1) / TILE;
    hipLaunchKernelGGL(bt_adapt_update_kernel, dim3(tiles_x * tiles_y), dim3(256), 0, stream, (const float4 *)rgba, moment, count,
                       active, error, n_active, width, height, tiles_x, T, p->threshold, p->min_samples, p->max_samples, p->eps);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_adapt_resolve(const float *rgba, const uint32_t *count, float *out, uint32_t width,
                                              uint32_t height, hipStream_t stream) {
    const uint32_t tiles_x = (width + TILE - 1) / TILE, n = width * height;
    hipLaunchKernelGGL(bt_adapt_resolve_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, (const float4 *)rgba, count,
                       (float4 *)out, width, height, tiles_x);
    return hipGetLastError();
}
