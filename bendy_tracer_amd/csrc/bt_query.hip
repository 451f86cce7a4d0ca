// bt_query.hip -- EXTENSION, NOT IN THE REFERENCE: the kernels of the ray query API (bt_query_rays_device, bt_view_rays_device;
// include/bendy_hip.h).
//
// bt_query_kernel is try_hit (tracer/mod.rs:389-402) for the caller's rays: one ray per lane, the row loop of the render
// kernels' generic build -- intersect_row() of bt_device.hpp, included read-only as tools/exact_math_check.hip includes it --
// over the scene's BtPrim table through the constant address space.  The row index is wave-uniform, so the rows arrive by scalar
// loads exactly as the render kernel gets them.  One build serves every scene.  After the loop each lane reads the row it hit
// (a per-lane load) and its refs from the table bt_api.cpp uploads next to the primitives (BtQueryRef).
//
// Memory access: a ray is 32 B and a hit 64 B per lane; stored straight from registers, each of a wave's 16-byte instructions
// would touch 64 separate records.  A workgroup's 256 records are staged through LDS instead: global memory sees 16 B per lane,
// 1 KiB contiguous per wave instruction, tails included; LDS holds the records by quarter (quarter k of record r at
// k * (256 + pad) + r) with the pad chosen so that both the per-record and the per-float4 side are free of bank conflicts
// (DESIGN.md 21 has the timing against the direct form).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bt_internal.hpp"
#include "bt_device.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr uint32_t kGroup = 256;
// float4 slots of the LDS stage: a ray is two quarters 256 + 8 apart, a hit four quarters 256 + 4 apart.  A float4 is four
// banks of 64: with these pads the 16 lanes of one ds_*_b128 phase, which hold 16 / quarters records times all their quarters
// on the global side, fall on 16 different groups of four banks (k * pad * 4 mod 64 = 32 k and 16 k).
constexpr uint32_t kRayPitch = kGroup + 8, kHitPitch = kGroup + 4;

} // namespace

__global__ __launch_bounds__(256) void bt_query_kernel(BtQueryLaunch Q) {
    __shared__ float4 stage[4 * kHitPitch];
    const uint32_t lane = threadIdx.x;
    const uint32_t base = blockIdx.x * kGroup;                 // < n < 2^30
    const uint32_t count = Q.n - base < kGroup ? Q.n - base : kGroup;   // records of this workgroup, >= 1

    // rays: global float4 g of the workgroup = quarter g & 1 of record g >> 1
    {
        const float4 *src = (const float4 *)Q.rays + (size_t)base * 2;
#pragma unroll
        for (uint32_t j = 0; j < 2; ++j) {
            const uint32_t g = lane + j * kGroup;
            if (g < 2 * count) stage[(g & 1u) * kRayPitch + (g >> 1)] = src[g];
        }
    }
    __syncthreads();
    // every lane of a tail wave stays alive through the loop (sqrt_bt holds a wave-uniform test): a lane without a record
    // takes the last one and stores nothing
    const uint32_t mine = lane < count ? lane : count - 1;
    const float4 r0 = stage[mine], r1 = stage[kRayPitch + mine];
    __syncthreads();                                           // the stage is reused for the hits

    V3 o = mk(r0.x, r0.y, r0.z), d = mk(r1.x, r1.y, r1.z);
    float tmin = r0.w, tmax = r1.w;
    // |v| < inf is false for NaN and for +-inf; tmax may be +inf but not NaN; tmin > tmax is an empty clip
    const float inf = __builtin_inff();
    const bool finite = fabsf(o.x) < inf && fabsf(o.y) < inf && fabsf(o.z) < inf && fabsf(d.x) < inf && fabsf(d.y) < inf &&
                        fabsf(d.z) < inf && fabsf(tmin) < inf;
    const bool valid = finite && tmax == tmax && !(tmin > tmax);
    if (!valid) {                                              // a ray that no row accepts; it is a miss whatever the loop says
        o = mk(0.0f, 0.0f, 0.0f);
        d = mk(0.0f, 0.0f, 0.0f);
        tmin = 1.0f;
        tmax = 0.0f;
    }

    HitRec h;
    h.t = tmax;
    h.prim = -1;
    h.inside = false;
    h.p_neg = false;
    BtPrimK *prims = (BtPrimK *)Q.prims;
    for (int i = 0; i < Q.n_prims; ++i) intersect_row<true, false>(prims, i, o, d, tmin, -1, h, false);

    float4 q0 = make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());                      // position, t
    float4 q1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));                    // normal, face
    uint64_t refs[3] = {~0ull, ~0ull, ~0ull};
    int prim = -1;
    if (valid && h.prim >= 0) {
        const BtPrim &R = Q.prims[h.prim];                     // per-lane row
        const BtQueryRef ref = Q.refs[h.prim];
        const V3 pos = o + d * h.t, c = mk(R.c);
        V3 normal;
        int face;
        if ((R.kind & BT_PRIM_SHAPE_MASK) == BT_PRIM_SPHERE) { // generate_surface_manifold (sphere.rs:85-119)
            const V3 e = pos - c;
            const V3 nrm = mk(e.x / R.radius, e.y / R.radius, e.z / R.radius);
            const bool front = dot(d, nrm) < 0.0f;
            normal = front ? nrm : -nrm;
            face = (R.volume >= 0 ? 3 : 0) + (front ? 0 : 1);
        } else {                                               // rect.rs:138-142
            normal = h.p_neg ? c : -c;
            face = h.p_neg ? 0 : 1;
        }
        q0 = make_float4(pos.x, pos.y, pos.z, h.t);
        q1 = make_float4(normal.x, normal.y, normal.z, __int_as_float(face));
        refs[0] = ref.object_ref;
        refs[1] = ref.material_ref;
        refs[2] = ref.volume_ref;
        prim = h.prim;
    }
    const float4 q2 = make_float4(__uint_as_float((uint32_t)refs[0]), __uint_as_float((uint32_t)(refs[0] >> 32)),
                                  __uint_as_float((uint32_t)refs[1]), __uint_as_float((uint32_t)(refs[1] >> 32)));
    const float4 q3 = make_float4(__uint_as_float((uint32_t)refs[2]), __uint_as_float((uint32_t)(refs[2] >> 32)),
                                  __int_as_float(prim), 0.0f);

    stage[lane] = q0;
    stage[kHitPitch + lane] = q1;
    stage[2 * kHitPitch + lane] = q2;
    stage[3 * kHitPitch + lane] = q3;
    __syncthreads();
    // hits: global float4 g of the workgroup = quarter g & 3 of record g >> 2; nothing beyond record count - 1 is written
    {
        float4 *dst = (float4 *)Q.hits + (size_t)base * 4;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t g = lane + j * kGroup;
            if (g < 4 * count) dst[g] = stage[(g & 3u) * kHitPitch + (g >> 2)];
        }
    }
}

// The rays through the footprint centres of a rectangle's pixels, row-major: btview::forward, the code the temporal stage
// reprojects with.  One ray per lane, two 16-byte stores.
__global__ __launch_bounds__(256) void bt_view_rays_kernel(BtViewRaysLaunch P) {
    const uint32_t i = blockIdx.x * kGroup + threadIdx.x;
    if (i >= P.w * P.h) return;
    const uint32_t x = P.x0 + i % P.w, y = P.y0 + i / P.w;
    float d[3];
    btview::forward(P.view, (float)x, (float)y, d);
    const float *T = P.view.v.to_world + 9;
    float4 *dst = (float4 *)P.rays + (size_t)i * 2;
    dst[0] = make_float4(T[0], T[1], T[2], P.view.v.clip_min);
    dst[1] = make_float4(d[0], d[1], d[2], P.view.v.clip_max);
}

// ---- host-side launchers (called from bt_query_api.cpp) ------------------------------------------------
extern "C" hipError_t bt_launch_query(const BtQueryLaunch *Q, hipStream_t stream) {
    hipLaunchKernelGGL(bt_query_kernel, dim3((Q->n + kGroup - 1) / kGroup), dim3(kGroup), 0, stream, *Q);
    return hipGetLastError();
}

extern "C" hipError_t bt_launch_view_rays(const BtViewRaysLaunch *P, hipStream_t stream) {
    hipLaunchKernelGGL(bt_view_rays_kernel, dim3((P->w * P->h + kGroup - 1) / kGroup), dim3(kGroup), 0, stream, *P);
    return hipGetLastError();
}
