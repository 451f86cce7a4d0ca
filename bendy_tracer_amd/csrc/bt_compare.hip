// bt_compare.hip -- EXTENSION, NOT IN THE REFERENCE: the kernels of the compare stage (bt_compare*): deterministic
// image-error metrics of a test frame against a reference frame, both w x h frames of running sums.
//
//   bt_compare_point_kernel   one thread per pixel, 16 x 16 workgroups (four waves of 64) on a one-dimensional grid of tiles.  Reads
//                             both frames as float4, writes (vx, vy) as one 16-byte store and E, and the tile's partials of se, re,
//                             valid, nonfinite and (m, index) into the slab's slot of the tile.
//   bt_compare_ssim_kernel    same tiling.  Stages the tile's 26 x 26 footprint of (vx, vy) in LDS, clamping as it stages, blurs
//                             the five products along x into a second LDS array (5 planes of 26 rows x 16 columns), blurs along
//                             y from there, writes s and the tile's partial.  29 504 B of LDS.
//   bt_compare_hist_kernel    one pass of the tail's radix select: a 2 048-bin integer histogram in LDS, flushed by integer atomics.
//   bt_compare_tail_kernel    same tiling as the point kernel: the tile's partials of S_gt, S_all and c_gt.
//   bt_compare_map_kernel     one thread per pixel: E -> RGBA8.
//
// The tile sums follow bt_compare.hpp's tree: strides 128 and 64 through LDS, strides 32 .. 1 inside wave 0 by cross-lane moves;
// t[k] + t[k + stride] is the same sum whichever operand arrives by which route.  The frame sums are formed on the host from the
// slab, in tile order.  There is no float atomic anywhere: the only atomics are the histogram's integer ones, which commute.
// Every thread of a workgroup reaches every barrier: one whose pixel lies outside the frame stages, waits, contributes 0.0 and
// skips only its stores.
#include <hip/hip_runtime.h>

#include <cstdint>

#define BT_COMPARE_LAUNCHERS
#include "bt_compare.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr uint32_t kTile = BT_COMPARE_TILE, kSpan = BT_COMPARE_SPAN, kThreads = kTile * kTile;
constexpr uint32_t kRows = kSpan * kTile;                      // entries of one row-blurred plane

// bt_compare.hpp's tile_tree over the workgroup's 256 slots; `t` is the thread's slot.  The sum is lane 0's (thread 0's).
__device__ inline double tile_sum(double *lds, double v, uint32_t t) {
    lds[t] = v;
    __syncthreads();
    if (t < 128u) lds[t] = lds[t] + lds[t + 128u];
    __syncthreads();
    double a = 0.0;
    if (t < 64u) {                                             // wave 0, all of it
        a = lds[t] + lds[t + 64u];
        a = a + __shfl_down(a, 32);
        a = a + __shfl_down(a, 16);
        a = a + __shfl_down(a, 8);
        a = a + __shfl_down(a, 4);
        a = a + __shfl_down(a, 2);
        a = a + __shfl_down(a, 1);
    }
    return a;
}

struct TileAt {
    uint32_t i, j, t;
    bool inside;
};
__device__ inline TileAt tile_at(uint32_t tiles_x, uint32_t w, uint32_t h) {
    TileAt a;
    a.i = (blockIdx.x % tiles_x) * kTile + threadIdx.x;
    a.j = (blockIdx.x / tiles_x) * kTile + threadIdx.y;
    a.t = threadIdx.y * kTile + threadIdx.x;
    a.inside = a.i < w && a.j < h;
    return a;
}

} // namespace

__global__ __launch_bounds__(256) void bt_compare_point_kernel(const float4 *__restrict__ X, float rx, const float4 *__restrict__ Y, float ry,
                                                               uint32_t w, uint32_t h, double epsilon, uint32_t tiles_x,
                                                               float *__restrict__ E, double2 *__restrict__ V, BtCompareSlab slab) {
    __shared__ double t_se[kThreads], t_re[kThreads], wave_m[4];
    __shared__ uint32_t wave_index[4], wave_valid[4], wave_bad[4];
    const TileAt at = tile_at(tiles_x, w, h);
    double se = 0.0, re = 0.0, m = 0.0;
    uint32_t index = 0xffffffffu;
    bool valid = false, bad = false;
    if (at.inside) {
        const size_t p = (size_t)at.j * w + at.i;
        const btcompare::Point pt = btcompare::point(X[p], rx, Y[p], ry, epsilon);
        E[p] = pt.E;
        V[p] = make_double2(pt.v.x, pt.v.y);
        se = pt.se;
        re = pt.re;
        m = pt.m;
        index = (uint32_t)p;
        bad = pt.bad;
        valid = !pt.bad;
    }
    // the integers: a ballot per wave for the counts, a butterfly for (m, index); any order gives the same pair
    const uint32_t n_valid = (uint32_t)__popcll(__ballot(valid)), n_bad = (uint32_t)__popcll(__ballot(bad));
    for (int s = 32; s >= 1; s >>= 1) {
        const double m2 = __shfl_xor(m, s);
        const uint32_t i2 = __shfl_xor(index, s);
        btcompare::max_merge(m, index, m2, i2);
    }
    const uint32_t wave = at.t / 64u;
    if (at.t % 64u == 0u) {
        wave_m[wave] = m;
        wave_index[wave] = index;
        wave_valid[wave] = n_valid;
        wave_bad[wave] = n_bad;
    }
    const double S_se = tile_sum(t_se, se, at.t), S_re = tile_sum(t_re, re, at.t);     // the barriers inside publish the wave_* too
    if (at.t == 0u) {
        uint32_t a = 0, b = 0;
        for (uint32_t k = 0; k < 4u; ++k) {
            a += wave_valid[k];
            b += wave_bad[k];
            if (k) btcompare::max_merge(m, index, wave_m[k], wave_index[k]);
        }
        slab.se[blockIdx.x] = S_se;
        slab.re[blockIdx.x] = S_re;
        slab.m[blockIdx.x] = m;
        slab.index[blockIdx.x] = index;
        slab.valid[blockIdx.x] = a;
        slab.nonfinite[blockIdx.x] = b;
    }
}

__global__ __launch_bounds__(256) void bt_compare_ssim_kernel(const double2 *__restrict__ V, uint32_t w, uint32_t h, uint32_t tiles_x,
                                                              double *__restrict__ S, BtCompareSlab slab) {
    __shared__ double2 stage[kSpan * kSpan];
    __shared__ double rows[5 * kRows];                         // planar: mx, my, xx, yy, xy, each 26 rows of 16
    __shared__ double t_s[kThreads];
    const TileAt at = tile_at(tiles_x, w, h);
    const uint32_t i0 = at.i - threadIdx.x, j0 = at.j - threadIdx.y;
    for (uint32_t e = at.t; e < kSpan * kSpan; e += kThreads) {
        const uint32_t a = e % kSpan, b = e / kSpan;
        stage[e] = V[(size_t)btcompare::stage_texel(j0, b, h) * w + btcompare::stage_texel(i0, a, w)];
    }
    __syncthreads();
    for (uint32_t e = at.t; e < kRows; e += kThreads) {
        const double2 *row = stage + (e / kTile) * kSpan + e % kTile;
        btcompare::Five acc = btcompare::five_zero();
#pragma unroll
        for (int k = 0; k < BT_COMPARE_TAPS; ++k) {
            const double2 v = row[k];
            btcompare::tap_pair(acc, btcompare::weight(k), btcompare::Pair{v.x, v.y});
        }
        rows[e] = acc.mx;
        rows[kRows + e] = acc.my;
        rows[2 * kRows + e] = acc.xx;
        rows[3 * kRows + e] = acc.yy;
        rows[4 * kRows + e] = acc.xy;
    }
    __syncthreads();
    btcompare::Five acc = btcompare::five_zero();
#pragma unroll
    for (int k = 0; k < BT_COMPARE_TAPS; ++k) {
        const double *q = rows + (threadIdx.y + k) * kTile + threadIdx.x;
        btcompare::tap_five(acc, btcompare::weight(k), btcompare::Five{q[0], q[kRows], q[2 * kRows], q[3 * kRows], q[4 * kRows]});
    }
    double s = 0.0;
    if (at.inside) {
        s = btcompare::ssim_of(acc);
        S[(size_t)at.j * w + at.i] = s;
    }
    const double S_s = tile_sum(t_s, s, at.t);
    if (at.t == 0u) slab.s[blockIdx.x] = S_s;
}

__global__ __launch_bounds__(256) void bt_compare_hist_kernel(const float *__restrict__ E, uint32_t n, uint32_t shift, uint32_t prefix_shift,
                                                              uint32_t prefix, uint32_t *__restrict__ hist) {
    __shared__ uint32_t bins[BT_COMPARE_BINS];
    for (uint32_t b = threadIdx.x; b < BT_COMPARE_BINS; b += 256u) bins[b] = 0u;
    __syncthreads();
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256u) {
        const uint32_t u = btcompare::bits_of(E[p]);
        if (btcompare::in_pass(u, prefix_shift, prefix)) atomicAdd(&bins[btcompare::bin_of(u, shift, prefix_shift)], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < BT_COMPARE_BINS; b += 256u)
        if (bins[b]) atomicAdd(&hist[b], bins[b]);
}

__global__ __launch_bounds__(256) void bt_compare_tail_kernel(const float *__restrict__ E, uint32_t w, uint32_t h, uint32_t tiles_x, float T,
                                                              BtCompareSlab slab) {
    __shared__ double t_gt[kThreads], t_all[kThreads];
    __shared__ uint32_t wave_gt[4];
    const TileAt at = tile_at(tiles_x, w, h);
    btcompare::TailTerm term{0.0, 0.0, 0u};
    if (at.inside) term = btcompare::tail_term(E[(size_t)at.j * w + at.i], T);
    const uint32_t n_gt = (uint32_t)__popcll(__ballot(term.c_gt != 0u));
    if (at.t % 64u == 0u) wave_gt[at.t / 64u] = n_gt;
    const double S_gt = tile_sum(t_gt, term.gt, at.t), S_all = tile_sum(t_all, term.all, at.t);
    if (at.t == 0u) {
        slab.gt[blockIdx.x] = S_gt;
        slab.all[blockIdx.x] = S_all;
        slab.c_gt[blockIdx.x] = (wave_gt[0] + wave_gt[1]) + (wave_gt[2] + wave_gt[3]);
    }
}

__global__ __launch_bounds__(256) void bt_compare_map_kernel(const float *__restrict__ E, uint32_t n, float scale, uint32_t *__restrict__ rgba8) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p < n) rgba8[p] = btcompare::map_pixel(E[p], scale);
}

// ---- host-side launchers (called from bt_compare_api.cpp; bt_compare.hpp declares them) ----------------------
namespace {

// the one-dimensional grid of 16 x 16 tiles; 0 for a frame whose tiles do not fit one launch (2^32 - 1 threads at most)
uint64_t tile_grid(uint32_t w, uint32_t h, uint32_t &tiles_x) {
    const uint64_t tx = btcompare::tiles_of(w), ty = btcompare::tiles_of(h);
    tiles_x = (uint32_t)tx;
    return tx * ty * kThreads > 0xffffffffull ? 0 : tx * ty;
}

} // namespace

extern "C" hipError_t bt_launch_compare_point(const float *X, float rx, const float *Y, float ry, uint32_t w, uint32_t h, double epsilon,
                                              float *E, double *V, BtCompareSlab slab, hipStream_t stream) {
    uint32_t tiles_x = 0;
    const uint64_t grid = tile_grid(w, h, tiles_x);
    if (!grid) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(bt_compare_point_kernel, dim3((uint32_t)grid), dim3(kTile, kTile), 0, stream, (const float4 *)X, rx, (const float4 *)Y, ry,
                       w, h, epsilon, tiles_x, E, (double2 *)V, slab);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_compare_ssim(const double *V, uint32_t w, uint32_t h, double *S, BtCompareSlab slab, hipStream_t stream) {
    uint32_t tiles_x = 0;
    const uint64_t grid = tile_grid(w, h, tiles_x);
    if (!grid) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(bt_compare_ssim_kernel, dim3((uint32_t)grid), dim3(kTile, kTile), 0, stream, (const double2 *)V, w, h, tiles_x, S, slab);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_compare_hist(const float *E, uint32_t n, uint32_t shift, uint32_t prefix_shift, uint32_t prefix,
                                             uint32_t *hist, hipStream_t stream) {
    const uint64_t blocks = ((uint64_t)n + 255u) / 256u;
    const uint32_t grid = blocks < 2048u ? (uint32_t)blocks : 2048u;      // the rest by the grid-stride loop
    hipLaunchKernelGGL(bt_compare_hist_kernel, dim3(grid), dim3(256), 0, stream, E, n, shift, prefix_shift, prefix, hist);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_compare_tail(const float *E, uint32_t w, uint32_t h, float T, BtCompareSlab slab, hipStream_t stream) {
    uint32_t tiles_x = 0;
    const uint64_t grid = tile_grid(w, h, tiles_x);
    if (!grid) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(bt_compare_tail_kernel, dim3((uint32_t)grid), dim3(kTile, kTile), 0, stream, E, w, h, tiles_x, T, slab);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_compare_map(const float *E, uint32_t n, float scale, uint8_t *rgba8, hipStream_t stream) {
    const uint64_t blocks = ((uint64_t)n + 255u) / 256u;
    if (blocks * 256u > 0xffffffffull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(bt_compare_map_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, E, n, scale, (uint32_t *)rgba8);
    return hipGetLastError();
}
