// bt_denoise.hip -- EXTENSION, NOT IN THE REFERENCE: kernels of the AOV-guided a-trous denoiser (bt_denoise*).
//
// Edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) on the albedo-demodulated colour (as in SVGF):
//   prepare  : running sums -> e = (C.rgb / n_c) / a' (alpha C.a rides along in e.w) and guide = (n.xyz, z)
//   pass i   : 5x5 taps at step 2^i, weight h[dx] h[dy] w_n w_z w_c, e_p <- sum w e_q / sum w (ping-pong buffers)
//   last pass: the same, then out.rgb = e * a' with a' recomputed from the albedo sums, out.a = e.w
// The tap order (dy outer, dx inner), the order of every product and sum and the -ffp-contract=off of the Makefile are the
// numerics contract: tests/denoise_ref.py restates them in float32 numpy, and the two differ by the ulps of expf / powf only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bt_internal.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int kTile = 16;          // 16 x 16 workgroups: 4 wave64, each wave a 16 x 4 strip of the frame

__device__ __forceinline__ float albedo_factor(float a, float eps) { return a > eps ? a : 1.0f; }

} // namespace

// One thread per pixel.  Missing guides are written as zeros: a zero normal on both ends of a tap and a zero depth
// difference give w_n = w_z = 1, so the pass kernel has no per-guide branches.
__global__ __launch_bounds__(256) void bt_denoise_prepare_kernel(const float4 *color, float nc, const float4 *albedo,
                                                                 float na, const float4 *normal, float nn,
                                                                 const float4 *depth, float nd, float eps_albedo,
                                                                 float4 *e_out, float4 *guide_out, uint32_t width,
                                                                 uint32_t height) {
    const uint32_t x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= width || y >= height) return;
    const size_t i = (size_t)y * width + x;
    const float4 C = color[i];
    float4 e = make_float4(C.x / nc, C.y / nc, C.z / nc, C.w);
    if (albedo) {
        const float4 A = albedo[i];
        e.x = e.x / albedo_factor(A.x / na, eps_albedo);
        e.y = e.y / albedo_factor(A.y / na, eps_albedo);
        e.z = e.z / albedo_factor(A.z / na, eps_albedo);
    }
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (normal) {
        const float4 N = normal[i];
        const float vx = N.x / nn, vy = N.y / nn, vz = N.z / nn;
        const float l2 = vx * vx + vy * vy + vz * vz;
        if (l2 > 1e-12f) {
            const float l = sqrtf(l2);
            g.x = vx / l;
            g.y = vy / l;
            g.z = vz / l;
        }
    }
    if (depth) g.w = depth[i].x / nd;
    e_out[i] = e;
    guide_out[i] = g;
}

// levels == 0: the mean itself, without the demodulation round trip.
__global__ __launch_bounds__(256) void bt_denoise_mean_kernel(const float4 *color, float nc, float4 *out, uint32_t width,
                                                              uint32_t height) {
    const uint32_t x = blockIdx.x * kTile + threadIdx.x, y = blockIdx.y * kTile + threadIdx.y;
    if (x >= width || y >= height) return;
    const size_t i = (size_t)y * width + x;
    const float4 C = color[i];
    out[i] = make_float4(C.x / nc, C.y / nc, C.z / nc, C.w);
}

// One a-trous level.  Per tap one 16-byte load of e and one of the guide; taps outside the frame drop out through the
// `inside` predicate (skipped, not clamped).  LAST: remodulate by a' and write the caller's frame instead of e.
template <bool LAST>
__global__ __launch_bounds__(256) void bt_denoise_pass_kernel(const float4 *__restrict__ e_in, const float4 *__restrict__ guide,
                                                              float4 *__restrict__ e_out, int step, float inv_color,
                                                              float sigma_normal, float sigma_depth,
                                                              const float4 *__restrict__ albedo, float na, float eps_albedo,
                                                              uint32_t width, uint32_t height) {
    const int x = (int)(blockIdx.x * kTile + threadIdx.x), y = (int)(blockIdx.y * kTile + threadIdx.y);
    const int W = (int)width, H = (int)height;
    if (x >= W || y >= H) return;
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const size_t ip = (size_t)y * W + x;
    const float4 ep = e_in[ip], gp = guide[ip];
    const bool np_zero = gp.x == 0.0f && gp.y == 0.0f && gp.z == 0.0f;
    const float zs = sigma_depth * gp.w * (float)step;      // sigma_depth * z_p * s, times max(|dx|, |dy|) below
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * step;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * step;
            const bool inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
            if (inside) {
                const size_t iq = (size_t)qy * W + qx;
                const float4 eq = e_in[iq], gq = guide[iq];
                const bool nq_zero = gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f;
                float wn;
                if (!np_zero && !nq_zero) {
                    const float d = gp.x * gq.x + gp.y * gq.y + gp.z * gq.z;
                    wn = powf(fmaxf(0.0f, d), sigma_normal);
                } else {
                    wn = np_zero && nq_zero ? 1.0f : 0.0f;
                }
                const int m = max(abs(dx), abs(dy));
                const float wz = expf(-fabsf(gp.w - gq.w) / (zs * (float)m + 1e-6f));
                const float dr = ep.x - eq.x, dg = ep.y - eq.y, db = ep.z - eq.z;
                const float wc = expf(-(dr * dr + dg * dg + db * db) * inv_color);
                const float w = h[dx + 2] * h[dy + 2] * wn * wz * wc;
                sr += w * eq.x;
                sg += w * eq.y;
                sb += w * eq.z;
                sw += w;
            }
        }
    }
    float4 r = make_float4(sr / sw, sg / sw, sb / sw, ep.w);
    if (LAST && albedo) {
        const float4 A = albedo[ip];
        r.x = r.x * albedo_factor(A.x / na, eps_albedo);
        r.y = r.y * albedo_factor(A.y / na, eps_albedo);
        r.z = r.z * albedo_factor(A.z / na, eps_albedo);
    }
    e_out[ip] = r;
}

// ---- host-side launchers (called from bt_denoise_api.cpp) ---------------------------------------------
// e0 / e1 / guide: the handle's scratch, width * height float4 each.  Enqueues levels + 1 kernels (1 for levels == 0).
extern "C" hipError_t bt_launch_denoise(const float *color, float nc, const float *albedo, float na, const float *normal,
                                        float nn, const float *depth, float nd, float *out, float *e0, float *e1,
                                        float *guide, uint32_t width, uint32_t height, uint32_t levels, float sigma_color,
                                        float sigma_normal, float sigma_depth, float eps_albedo, hipStream_t stream) {
    const dim3 grid((width + kTile - 1) / kTile, (height + kTile - 1) / kTile), block(kTile, kTile);
    if (levels == 0) {
        hipLaunchKernelGGL(bt_denoise_mean_kernel, grid, block, 0, stream, (const float4 *)color, nc, (float4 *)out, width,
                           height);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(bt_denoise_prepare_kernel, grid, block, 0, stream, (const float4 *)color, nc,
                       (const float4 *)albedo, na, (const float4 *)normal, nn, (const float4 *)depth, nd, eps_albedo,
                       (float4 *)e0, (float4 *)guide, width, height);
    hipError_t err = hipGetLastError();
    const float sc2 = sigma_color * sigma_color;
    float *src = e0, *dst = e1;
    for (uint32_t i = 0; i < levels && err == hipSuccess; ++i) {
        const float inv_color = (float)(1u << (2 * i)) / sc2;       // 4^i / sigma_color^2, f32 on the host
        const int step = 1 << i;
        if (i + 1 < levels) {
            hipLaunchKernelGGL(bt_denoise_pass_kernel<false>, grid, block, 0, stream, (const float4 *)src,
                               (const float4 *)guide, (float4 *)dst, step, inv_color, sigma_normal, sigma_depth,
                               (const float4 *)nullptr, na, eps_albedo, width, height);
        } else {
            hipLaunchKernelGGL(bt_denoise_pass_kernel<true>, grid, block, 0, stream, (const float4 *)src,
                               (const float4 *)guide, (float4 *)out, step, inv_color, sigma_normal, sigma_depth,
                               (const float4 *)albedo, na, eps_albedo, width, height);
        }
        err = hipGetLastError();
        float *t = src;
        src = dst;
        dst = t;
    }
    return err;
}
