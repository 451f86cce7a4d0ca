// bt_temporal.hip -- EXTENSION, NOT IN THE REFERENCE: the kernel of temporal accumulation with reprojection (bt_temporal*,
// DESIGN.md 14).
//
// One thread per pixel, one launch per frame: prepare the pixel's mean colour, normal and depth from this frame's running
// sums, find where the pixel's point was in the previous view (bt_view.hpp), gather the previous history bilinearly with a
// depth and a normal test per tap, blend, and write the caller's frame, the new history plane and the new guide plane.
// The order of every product and sum and the -ffp-contract=off of the Makefile are what tests/temporal_ref.py restates in
// float32 numpy; the two differ by the ulps of sinf / cosf / asinf / atan2f only (the static path has none of them).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bt_internal.hpp"
#include "bt_view.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int kTile = 16;          // 16 x 16 workgroups: 4 wave64, each wave a 16 x 4 strip of the frame

// s = the surviving taps' weighted history (rgb, length), sw their weight: the blended pixel and its new history length
__device__ __forceinline__ float4 blend(float4 s, float sw, float cr, float cg, float cb, const BtTemporalLaunch &P) {
    const float mr = s.x / sw, mg = s.y / sw, mb = s.z / sw, h = s.w / sw;
    const float N = fminf(h + P.nc, P.max_history);
    const float a = fminf(1.0f, fmaxf(P.nc / N, P.alpha_min));
    return make_float4(mr + (cr - mr) * a, mg + (cg - mg) * a, mb + (cb - mb) * a, N);
}

} // namespace

// MODE 0: no history (every pixel is reset); 1: the view is the previous one, the pixel's own history is taken; 2: reproject.
template <int MODE>
__global__ __launch_bounds__(256) void bt_temporal_kernel(BtTemporalLaunch P) {
    const int x = (int)(blockIdx.x * kTile + threadIdx.x), y = (int)(blockIdx.y * kTile + threadIdx.y);
    const int W = (int)P.cur.v.width, H = (int)P.cur.v.height;
    if (x >= W || y >= H) return;
    const size_t ip = (size_t)y * W + x;
    const float4 C = P.color[ip];
    const float cr = C.x / P.nc, cg = C.y / P.nc, cb = C.z / P.nc;
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (P.normal) {                                        // bt_denoise_prepare_kernel's normal
        const float4 N = P.normal[ip];
        const float vx = N.x / P.nn, vy = N.y / P.nn, vz = N.z / P.nn;
        const float l2 = vx * vx + vy * vy + vz * vz;
        if (l2 > 1e-12f) {
            const float l = sqrtf(l2);
            g.x = vx / l;
            g.y = vy / l;
            g.z = vz / l;
        }
    }
    g.w = P.depth[ip].x / P.nd;
    const bool far = g.w >= 1.0f;

    float4 r = make_float4(cr, cg, cb, P.nc);              // a reset: the frame's own mean, history length n_c
    if (MODE == 1) {
        // the pose the history was taken from, and a static world: the pixel sees what it saw, so its own history is taken
        // as it is, without the tests -- the running mean, also on a silhouette whose samples hit in one frame and miss in the next
        r = blend(P.hist_in[ip], 1.0f, cr, cg, cb, P);
    }
    if (MODE == 2) {
        float o[3];
        btview::reproject(P.cur, P.prev, (float)x, (float)y, g.w, o);
        const float xf = o[0], yf = o[1], zp = o[2];
        // a non-finite position fails the comparisons: outside the frame, like every position a whole pixel beyond its edge
        if (xf > -1.0f && xf < (float)W && yf > -1.0f && yf < (float)H) {
            const float x0f = floorf(xf), y0f = floorf(yf);
            const float fx = xf - x0f, fy = yf - y0f;
            const int x0 = (int)x0f, y0 = (int)y0f;        // -1 .. W - 1, -1 .. H - 1
            const bool np_zero = g.x == 0.0f && g.y == 0.0f && g.z == 0.0f;
            const float ztol = P.depth_tolerance * zp;
            float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float sw = 0.0f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int qx = x0 + i, qy = y0 + j;
                    const float w = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                    const bool inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
                    if (inside && w != 0.0f) {             // the address is formed for taps inside the plane only
                        const size_t iq = (size_t)qy * W + qx;
                        const float4 gq = P.guide_in[iq];
                        const bool pass_z = far ? gq.w >= 1.0f : (gq.w < 1.0f && fabsf(zp - gq.w) <= ztol);
                        bool pass_n = true;
                        if (P.normal) {
                            const bool nq_zero = gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f;
                            if (np_zero || nq_zero) pass_n = np_zero && nq_zero;
                            else pass_n = (g.x * gq.x + g.y * gq.y) + g.z * gq.z >= P.normal_min;
                        }
                        if (pass_z && pass_n) {
                            const float4 hq = P.hist_in[iq];
                            s.x += w * hq.x;
                            s.y += w * hq.y;
                            s.z += w * hq.z;
                            s.w += w * hq.w;
                            sw += w;
                        }
                    }
                }
            }
            if (sw >= 1e-3f) r = blend(s, sw, cr, cg, cb, P);
        }
    }
    P.out[ip] = make_float4(r.x, r.y, r.z, C.w);
    P.hist_out[ip] = r;
    P.guide_out[ip] = g;
}

// ---- host-side launcher (called from bt_temporal_api.cpp) ------------------------------------------------
extern "C" hipError_t bt_launch_temporal(const BtTemporalLaunch *P, int mode, hipStream_t stream) {
    const uint32_t width = P->cur.v.width, height = P->cur.v.height;
    const dim3 grid((width + kTile - 1) / kTile, (height + kTile - 1) / kTile), block(kTile, kTile);
    if (mode == 0) hipLaunchKernelGGL(bt_temporal_kernel<0>, grid, block, 0, stream, *P);
    else if (mode == 1) hipLaunchKernelGGL(bt_temporal_kernel<1>, grid, block, 0, stream, *P);
    else hipLaunchKernelGGL(bt_temporal_kernel<2>, grid, block, 0, stream, *P);
    return hipGetLastError();
}
