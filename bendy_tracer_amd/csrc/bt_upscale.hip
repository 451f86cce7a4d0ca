// bt_upscale.hip -- EXTENSION, NOT IN THE REFERENCE: the kernels of the upscale stage (bt_upscale*): joint bilateral
// upsampling of a w x h frame of colour sums to a W x H mean, steered by the albedo, normal and depth guides of both sizes.
//
//   bt_upscale_prepare_kernel   one thread per lo texel: reads the colour sums and the present lo guides once and writes the three
//                               prepared planes (c.rgb, z), (n.xyz, 0), (a.rgb, 0).  An absent guide is written as zeros, which
//                               weigh exactly 1 against the zeros the main kernel takes for its hi side: no per-guide branch
//                               in the tap loop.
//   bt_upscale_kernel<staged>   one thread per output pixel, 16 x 16 workgroups on a one-dimensional grid of tiles.  A thread
//                               prepares its own hi guides in registers and walks bt_upscale.hpp's 16 taps, unrolled.
// The staged form (the product build; -DBT_UPSCALE_LDS=0 builds the direct one) uses that the 16 outputs of a tile take at most
// 15 + 4 = 19 source texels per axis when dst >= src: the 19 x 19 footprint of the three planes goes into LDS (17 328 B), clamped
// as it is staged, and a tap is three 16-byte LDS reads at (first_i - first_i0 + tx, first_j - first_j0 + ty).  The direct form
// clamps and loads from the planes per tap.  Both run bt_upscale.hpp's pixel() over the same texels in the same order.
// Every thread of a workgroup reaches both barriers: one whose pixel lies outside the frame stages, waits and skips the store.
// The two counters take one 64-bit atomic per workgroup (tier 2 in the low word, tier 3 in the high one) after a ballot per wave.
#include <hip/hip_runtime.h>

#include <cstdint>

#define BT_UPSCALE_LAUNCHERS
#include "bt_upscale.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr uint32_t kTile = BT_UPSCALE_TILE, kSpan = BT_UPSCALE_SPAN;

// Output pixel (i, j), inside the frame: its own hi guides prepared in registers, its eight weights of each axis as two 16-byte
// loads, the alpha of the nearest colour texel, then bt_upscale.hpp's pixel() over the taps that `fetch` hands out.
template <class F>
__device__ inline float4 upscale_one(F fetch, const float4 *__restrict__ colour, uint32_t w, const BtUpscaleGuides &hi, uint32_t W,
                                     const BtUpscaleAxis &ax, const BtUpscaleAxis &ay, const btupscale::Weights &P, uint32_t i, uint32_t j,
                                     int &tier) {
    const size_t p = (size_t)j * W + i;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 n = hi.normal ? btupscale::prepare_normal(((const float4 *)hi.normal)[p], hi.r_normal) : zero;
    const float4 a = hi.albedo ? btupscale::prepare_albedo(((const float4 *)hi.albedo)[p], hi.r_albedo) : zero;
    const float z = hi.depth ? btupscale::prepare_depth(((const float4 *)hi.depth)[p].x, hi.r_depth) : 0.0f;
    const float4 *wx = (const float4 *)ax.weights + (size_t)i * 2, *wy = (const float4 *)ay.weights + (size_t)j * 2;
    const float4 x1 = wx[0], x2 = wx[1], y1 = wy[0], y2 = wy[1];
    const float ux[8] = {x1.x, x1.y, x1.z, x1.w, x2.x, x2.y, x2.z, x2.w}, uy[8] = {y1.x, y1.y, y1.z, y1.w, y2.x, y2.y, y2.z, y2.w};
    const float alpha = colour[(size_t)ay.nearest[j] * w + ax.nearest[i]].w;
    return btupscale::pixel<float4>(fetch, btupscale::centre_of(n, a, z, P), ux, uy, P, alpha, tier);
}

} // namespace

__global__ __launch_bounds__(256) void bt_upscale_prepare_kernel(const float4 *__restrict__ colour, float r, float max_value,
                                                                 BtUpscaleGuides lo, uint32_t texels, float4 *__restrict__ planes) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= texels) return;
    const float z = lo.depth ? btupscale::prepare_depth(((const float4 *)lo.depth)[i].x, lo.r_depth) : 0.0f;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    planes[i] = btupscale::prepare_colour(colour[i], r, max_value, z);
    planes[(size_t)texels + i] = lo.normal ? btupscale::prepare_normal(((const float4 *)lo.normal)[i], lo.r_normal) : zero;
    planes[2 * (size_t)texels + i] = lo.albedo ? btupscale::prepare_albedo(((const float4 *)lo.albedo)[i], lo.r_albedo) : zero;
}

template <bool kStaged>
__global__ __launch_bounds__(256) void bt_upscale_kernel(const float4 *__restrict__ planes, const float4 *__restrict__ colour, uint32_t w,
                                                         uint32_t h, BtUpscaleGuides hi, float4 *__restrict__ out, uint32_t W, uint32_t H,
                                                         BtUpscaleAxis ax, BtUpscaleAxis ay, btupscale::Weights P, uint32_t tiles_x,
                                                         unsigned long long *__restrict__ counters) {
    __shared__ uint32_t wave_counts[2 * 8];           // four waves of 64 lanes; room for eight of 32
    const uint32_t i0 = (blockIdx.x % tiles_x) * kTile, j0 = (blockIdx.x / tiles_x) * kTile;
    const uint32_t i = i0 + threadIdx.x, j = j0 + threadIdx.y, t = threadIdx.y * kTile + threadIdx.x;
    const bool inside = i < W && j < H;
    // a thread outside the frame reads the tables of the frame's last column / row: no address outside a table is formed
    const uint32_t ic = i < W ? i : W - 1u, jc = j < H ? j : H - 1u;
    const size_t texels = (size_t)w * h;
    const float4 *pcz = planes, *pn = planes + texels, *pa = planes + 2 * texels;
    const int32_t fx = ax.first[ic], fy = ay.first[jc];

    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int tier = 0;
    if constexpr (kStaged) {
        __shared__ float4 stage[3 * kSpan * kSpan];
        const int32_t fx0 = ax.first[i0], fy0 = ay.first[j0];      // i0 < W and j0 < H: the grid covers the frame only
        for (uint32_t e = t; e < kSpan * kSpan; e += kTile * kTile) {
            const uint32_t a = e % kSpan, b = e / kSpan;
            const size_t q = (size_t)btupscale::clamp_index((int64_t)fy0 + b, h) * w + btupscale::clamp_index((int64_t)fx0 + a, w);
            stage[e] = pcz[q];
            stage[kSpan * kSpan + e] = pn[q];
            stage[2 * kSpan * kSpan + e] = pa[q];
        }
        __syncthreads();
        if (inside) {
            // the tables never decrease, so 0 <= fx - fx0 <= 15; the bound keeps a stray table inside the stage
            const uint32_t ox = (uint32_t)(fx - fx0) <= kSpan - 4u ? (uint32_t)(fx - fx0) : kSpan - 4u;
            const uint32_t oy = (uint32_t)(fy - fy0) <= kSpan - 4u ? (uint32_t)(fy - fy0) : kSpan - 4u;
            const float4 *mine = stage + oy * kSpan + ox;
            o = upscale_one(
                [&](int tx, int ty, float4 &qcz, float4 &qn, float4 &qa) {
                    const float4 *q = mine + ty * (int)kSpan + tx;
                    qcz = q[0];
                    qn = q[kSpan * kSpan];
                    qa = q[2 * kSpan * kSpan];
                },
                colour, w, hi, W, ax, ay, P, i, j, tier);
        }
    } else {
        if (inside)
            o = upscale_one(
                [&](int tx, int ty, float4 &qcz, float4 &qn, float4 &qa) {
                    const size_t q = (size_t)btupscale::clamp_index((int64_t)fy + ty, h) * w + btupscale::clamp_index((int64_t)fx + tx, w);
                    qcz = pcz[q];
                    qn = pn[q];
                    qa = pa[q];
                },
                colour, w, hi, W, ax, ay, P, i, j, tier);
    }
    if (inside) out[(size_t)j * W + i] = o;
    // the counters: a ballot per wave, one atomic per workgroup
    const uint32_t n2 = (uint32_t)__popcll(__ballot(tier == 2)), n3 = (uint32_t)__popcll(__ballot(tier == 3));
    const uint32_t wave = t / warpSize, waves = kTile * kTile / warpSize;
    if (t % warpSize == 0) {
        wave_counts[2 * wave] = n2;
        wave_counts[2 * wave + 1] = n3;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t a = 0, b = 0;
        for (uint32_t k = 0; k < waves; ++k) {
            a += wave_counts[2 * k];
            b += wave_counts[2 * k + 1];
        }
        // neither count can exceed the pixel count, which is below 2^32
        if (a | b) atomicAdd(counters, (unsigned long long)a | ((unsigned long long)b << 32));
    }
}

// ---- host-side launchers (called from bt_upscale_api.cpp, which declares them too) --------------------------
extern "C" hipError_t bt_launch_upscale_prepare(const float *colour, float r, float max_value, BtUpscaleGuides lo, uint32_t w, uint32_t h,
                                                float *planes, hipStream_t stream) {
    const uint64_t texels = (uint64_t)w * h;
    if (texels > 0xffffffffull) return hipErrorInvalidConfiguration;
    const uint32_t grid = (uint32_t)((texels + 255u) / 256u);
    hipLaunchKernelGGL(bt_upscale_prepare_kernel, dim3(grid), dim3(256), 0, stream, (const float4 *)colour, r, max_value, lo, (uint32_t)texels,
                       (float4 *)planes);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_upscale(const float *planes, const float *colour, uint32_t w, uint32_t h, BtUpscaleGuides hi, float *out,
                                        uint32_t W, uint32_t H, BtUpscaleAxis ax, BtUpscaleAxis ay, btupscale::Weights P,
                                        unsigned long long *counters, hipStream_t stream) {
    const uint64_t tx = ((uint64_t)W + kTile - 1) / kTile, ty = ((uint64_t)H + kTile - 1) / kTile;
    if (tx * ty * 256 > 0xffffffffull) return hipErrorInvalidConfiguration;        // the runtime takes at most 2^32 - 1 threads per launch
    if (W < w || H < h) return hipErrorInvalidValue;                               // the staged footprint holds for dst >= src only
    hipLaunchKernelGGL(bt_upscale_kernel<BT_UPSCALE_LDS != 0>, dim3((uint32_t)(tx * ty)), dim3(kTile, kTile), 0, stream, (const float4 *)planes,
                       (const float4 *)colour, w, h, hi, (float4 *)out, W, H, ax, ay, P, (uint32_t)tx, counters);
    return hipGetLastError();
}
