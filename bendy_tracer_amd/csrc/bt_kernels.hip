// bt_kernels.hip -- gfx950 (MI355X / CDNA4) kernels for bendy-tracer's per-sample hot path.
//
// One launch of bt_render_kernel computes Tracer::render (reference tracer/mod.rs:179-202)
// for every pixel of the frame (or of this rank's tile shard):
//   camera ray (mod.rs:271-302) -> iterative form of sample / sample_surface /
//   sample_volume / sample_volumetric / sample_root (mod.rs:322-523) with
//   try_hit / try_hit_volume over the flattened primitive table (mod.rs:389-427,
//   sphere.rs, rect.rs, cuboid.rs), material shading (material.rs) and the density-map
//   march (volume.rs) -> `+=` into the RGBA32F accumulator (buffer.rs:159-178).
//
// Mapping to the hardware:
//   * a workgroup owns a block of 256/S pixels (S = 1..32) and all of their samples in this launch.  The block's
//     (pixel, sample) pairs are a work queue in LDS: a lane whose path has ended takes the next pair, every sample's
//     value is parked in HBM and the last wave of the workgroup adds the parked values to the frame in sample order --
//     the reference's per-pixel summation order, no atomics on the frame;
//   * a launch of only a few work items per lane of the GPU is PACKED instead: one workgroup per workgroup slot, each
//     owning every k-th pixel block behind one queue, so that the GPU drains its longest paths once, not once per
//     generation of workgroups (own builds, template flag PACKED);
//   * in the sphere-only builds a wave votes every iteration whether it runs the camera event or the scatter / volume
//     events; the lanes of the other kind keep their state for the next iteration (phase voting);
//   * every loop iteration is TRACE (one path segment, all lanes) followed by exactly ONE random event per lane --
//     a Diffuse / Metallic / Glass scatter, a volume step, or, for a lane whose path just ended, the camera ray of
//     its next sample.  The event's Philox block, its sin/cos, its basis construction and its final normalize are
//     shared by all event kinds, so those instructions run with every lane active; a wave never idles on its
//     longest path;
//   * the primitive table is read with wave-uniform indices through the constant address space -> scalar (SMEM)
//     loads that broadcast through SGPRs; per-lane lookups (hit primitive, material, light, density) go to tables
//     staged in LDS; the camera block of the launch parameters is read where it is used, not kept in SGPRs;
//   * template flags select a build without rect code / without the volume march for scenes that have neither;
//   * sphere-only launches without volumes: bt_block_mask_kernel (one thread per pixel block, double precision,
//     bt_cull.hpp) writes which sphere rows each block's camera rays can reach, bt_block_order_kernel lists the blocks that
//     can reach any ahead of those that reach none, bt_api.cpp keeps both on the scene handle for as long as their inputs
//     stay the same; the render kernel's first workgroups trace the listed blocks, the next few add the background's value
//     to the pixels of the empty ones -- 256 pixels each, nothing traced -- and the rest return at once;
//   * no MFMA: there is no dense contraction on this path.
//
// Round 3 removed what had lost every measurement of rounds 1 and 2 (the logs stay under profiles/): the lane-owns-pixel
// mapping, the streaming queue with its ring of parked units, the regrouping kernel (bt_kernels_sorted.hip) and the A/B
// knobs BT_VOTE3, BT_VOTE_SOFT_K, BT_XCD_ROTATE, BT_PK_PAIRS, BT_WG_THREADS, BT_VOTE_RECTS, BT_NUM_SGPR, BT_WAVES_EXACT.
// Round 3's own experiments are gone again too, each bit-exact and each measured slower or no faster: persistent workgroups
// that claim pixel blocks with the sums in a second kernel (profiles/r04b), a pool of path records in LDS through which paths
// change lanes -- a "march stack" for paths that enter a volume (profiles/r04d) and end-of-block compaction (profiles/r04c,
// r04e, r04f).
#include "bt_device.hpp"
#include "bt_color.hpp"
#include "bt_cull.hpp"
#include "bt_internal.hpp"

#define BT_SUM_BATCH 8             // parked values a lane of the summing wave has in flight (16: no difference, profiles/r04k)

// Developer build (-DBT_PROFILE): s_memtime stamps around the sections of the render loop, summed per wave into
// counters[2..]; shares of wave cycles are printed by bt_scene_last_stats.  Not part of the product build.
// Developer build (-DBT_LANESTAT, implies the 12 counters of BT_PROFILE): per wave-iteration popcounts of what the lanes
// do, summed into counters[2..]: [2] wave iterations, [3] lanes that trace, [4..8] lanes per event kind (camera, Diffuse,
// Metallic, Glass, volume), [9] lanes waiting for their phase, [10] lanes that have left the loop (queue empty).
#ifdef BT_LANESTAT
#define BT_LS(i, mask) do { ls_acc[i] += (unsigned long long)__popcll(mask); } while (0)   // every lane still in the loop counts; max over lanes at the end
#else
#define BT_LS(i, mask)
#endif
#ifdef BT_PROFILE
#define BT_PROF_DECL unsigned long long prof_t = __builtin_readcyclecounter(), prof_acc[BT_N_COUNTERS - 2] = {}
#define BT_PROF(i) do { const unsigned long long now_ = __builtin_readcyclecounter(); prof_acc[i] += now_ - prof_t; prof_t = now_; } while (0)
#else
#define BT_PROF_DECL
#define BT_PROF(i)
#endif

namespace {

// A parked sample value: 12 bytes (round 1 parked a float4 with an unused w -- a quarter of the block queue's HBM traffic).
struct Parked { float x, y, z; };
// Guided render (EXTENSION, OUTPUT == 4): a parked depth value -- one float, added to all three channels (buffer.rs:172-178)
struct Parked1 { float x; };
BT_DEV V3 v3_of(const Parked &v) { return mk(v.x, v.y, v.z); }
BT_DEV V3 v3_of(const Parked1 &v) { return mk(v.x, v.x, v.x); }
BT_DEV V3 shfl_v3(const Parked &v, int from) { return mk(__shfl(v.x, from, 64), __shfl(v.y, from, 64), __shfl(v.z, from, 64)); }
BT_DEV V3 shfl_v3(const Parked1 &v, int from) { const float d = __shfl(v.x, from, 64); return mk(d, d, d); }

enum { EV_GEN = 0, EV_DIFFUSE = 1, EV_METALLIC = 2, EV_GLASS = 3, EV_VOLUME = 4 };

// A path in flight, as it changes lanes in the drain of a packed launch (80 bytes): ray, throughput, radiance; event counter,
// pixel, work item; bounce | volume bounce << 16; in-volume object + 1 | vote wait << 24 | held << 31; the held hit.
struct __attribute__((aligned(16))) PathRec { float f[12]; uint32_t w[8]; };

// lanes of a wave64 mask below this lane
BT_DEV uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// (where a pixel block lies in the frame: block_geom, block_ref, block_extent of bt_cull.hpp, shared with the mask kernel and the host)
// pixel q of a block: quadrants 1 .. 3 of a 128- or 256-pixel block sit to the right of / below quadrant 0
struct PixelRef { uint32_t px, py; bool in_frame; };
BT_DEV PixelRef pixel_of(const BtLaunch &P, const BlockGeom &g, const BlockRef &B, uint32_t q) {
    PixelRef r;
    r.px = B.px0 + (q & g.WMASK) + ((q >> 3) & 8u);
    r.py = B.py0 + ((q & 63u) >> g.LBW) + ((q >> 4) & 8u);
    r.in_frame = B.tile_ok && r.px < P.width && r.py < P.height;
    return r;
}
// the pixel's running sum: row-major frame, or this rank's tile-major shard
// (`frame` = BtLaunch::out, or one of the guide frames of a guided render)
BT_DEV float *out_of(const BtLaunch &P, float *frame, const BlockRef &B, const PixelRef &r) {
    return P.sharded ? frame + ((size_t)B.slot * (BT_TILE_DIM * BT_TILE_DIM) + (r.py & 15u) * BT_TILE_DIM + (r.px & 15u)) * 4
                     : frame + ((size_t)r.py * P.width + r.px) * 4;
}

// Adaptive sampling (EXTENSION, OUTPUT == 5): a sample's contribution to its pixel's second moment -- the square of its
// Rec. 709 luminance, added in sample order next to the colour (bt_adapt.hip turns sum and moment into the tile's error)
BT_DEV float moment_add(float m, const V3 &v) {
    const float Y = (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z;
    return m + Y * Y;
}

// `*r += pixel.r` (buffer.rs:159-164) for every parked sample of block b's pixels, in sample order -- the additions a
// lane that owned the pixel would perform in a register, in the same order, hence the same bits.  Executed by ONE wave
// (`lane` = 0 .. 63); src = the block's parked values, src[k * pxb + pixel].
// PK = Parked, or Parked1 for the depth plane of a guided render; `frame` = the frame the plane is added to.
// MOMENT (adaptive builds): the wave also adds every value's squared luminance to moment[py * width + px], in the same order.
template <class PK, bool MOMENT = false>
BT_DEV void sum_block(const BtLaunch &P, const BlockGeom &g, uint32_t b, uint32_t T, const PK *src, uint32_t lane, float *frame,
                      float *moment = nullptr) {
    const BlockRef B = block_ref(P, g, b);
    const uint32_t pxb = g.pxb;
    if (pxb >= 64) {
        for (uint32_t q = lane; q < pxb; q += 64) {
            const PixelRef r = pixel_of(P, g, B, q);
            if (!r.in_frame) continue;
            float *o = out_of(P, frame, B, r);
            const PK *s = src + q;
            V3 sum = mk(o[0], o[1], o[2]);
            float *mo = nullptr;
            float m = 0.0f;
            if constexpr (MOMENT) {
                mo = moment + ((size_t)r.py * P.width + r.px);
                m = *mo;
            }
            uint32_t kk = 0;
            for (; kk + BT_SUM_BATCH <= T; kk += BT_SUM_BATCH) {   // BT_SUM_BATCH loads in flight, additions strictly in order
                PK v[BT_SUM_BATCH];
#pragma unroll
                for (int j = 0; j < BT_SUM_BATCH; ++j) v[j] = s[(size_t)(kk + j) * pxb];
#pragma unroll
                for (int j = 0; j < BT_SUM_BATCH; ++j) {
                    sum = sum + v3_of(v[j]);
                    if constexpr (MOMENT) m = moment_add(m, v3_of(v[j]));
                }
            }
            for (; kk < T; ++kk) {
                const PK v = s[(size_t)kk * pxb];
                sum = sum + v3_of(v);
                if constexpr (MOMENT) m = moment_add(m, v3_of(v));
            }
            o[0] = sum.x;
            o[1] = sum.y;
            o[2] = sum.z;
            if constexpr (MOMENT) *mo = m;
        }
    } else {
        // 32, 16 or 8 pixels (deep launches, T in the hundreds): J = 64 / pxb lanes per pixel fetch interleaved
        // samples (8 J in flight per pixel), lane (q, 0) adds them in sample order out of the others' registers
        const uint32_t J = 64u >> g.LOG_PXB, q = lane & (pxb - 1u), jl = lane >> g.LOG_PXB;
        const PixelRef r = pixel_of(P, g, B, q);
        const bool owner = jl == 0 && r.in_frame;
        float *o = out_of(P, frame, B, r);
        const PK *s = src + q;
        V3 sum = mk(0.0f, 0.0f, 0.0f);
        if (owner) sum = mk(o[0], o[1], o[2]);
        float *mo = nullptr;
        float m = 0.0f;
        if constexpr (MOMENT) {
            mo = moment + ((size_t)r.py * P.width + r.px);
            if (owner) m = *mo;
        }
        for (uint32_t kk = 0; kk < T; kk += 8 * J) {
            PK v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint32_t k2 = kk + (uint32_t)u * J + jl;
                v[u] = k2 < T ? s[(size_t)k2 * pxb] : PK{};
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                for (uint32_t jj = 0; jj < J; ++jj) {
                    const int from = (int)(q + jj * pxb);
                    const V3 val = shfl_v3(v[u], from);
                    if (kk + (uint32_t)u * J + jj < T) {
                        sum = sum + val;
                        if constexpr (MOMENT) m = moment_add(m, val);
                    }
                }
        }
        if (owner) {
            o[0] = sum.x;
            o[1] = sum.y;
            o[2] = sum.z;
            if constexpr (MOMENT) *mo = m;
        }
    }
}


// A workgroup of a packed launch (BtLaunch::wg_blocks > 1) owns the blocks first, first + stride, ...: `n` of them, parked
// back to back.  All its threads sum, one pixel each at a time, BT_SUM_BATCH parked values in flight, additions strictly in
// sample order.
template <class PK>
BT_DEV void sum_blocks(const BtLaunch &P, const BlockGeom &g, uint32_t first, uint32_t stride, uint32_t n, uint32_t T,
                       const PK *src, uint32_t thread, uint32_t n_threads, float *frame) {
    const uint32_t LOG_ROWS = P.log_rows;              // a block's samples are padded to 2^log_rows rows of pxb parked values
    for (uint32_t p = thread; p < (n << g.LOG_PXB); p += n_threads) {
        const uint32_t j = p >> g.LOG_PXB, q = p & (g.pxb - 1u);
        const BlockRef B = block_ref(P, g, first + j * stride);
        const PixelRef r = pixel_of(P, g, B, q);
        if (!r.in_frame) continue;
        float *o = out_of(P, frame, B, r);
        const PK *s = src + ((size_t)j << (LOG_ROWS + g.LOG_PXB)) + q;
        V3 sum = mk(o[0], o[1], o[2]);
        uint32_t kk = 0;
        for (; kk + BT_SUM_BATCH <= T; kk += BT_SUM_BATCH) {
            PK v[BT_SUM_BATCH];
#pragma unroll
            for (int u = 0; u < BT_SUM_BATCH; ++u) v[u] = s[(size_t)(kk + u) << g.LOG_PXB];
#pragma unroll
            for (int u = 0; u < BT_SUM_BATCH; ++u) sum = sum + v3_of(v[u]);
        }
        for (; kk < T; ++kk) {
            const PK v = s[(size_t)kk << g.LOG_PXB];
            sum = sum + v3_of(v);
        }
        o[0] = sum.x;
        o[1] = sum.y;
        o[2] = sum.z;
    }
}

// Blocks whose mask is empty: every sample of such a block is one segment that misses, its value is sample_root's with the
// camera's beta and L.  A fill workgroup takes 256 >> LOG_PXB = `slices` of them, so that each of its 256 threads has one
// pixel: thread t pixel t & (pxb - 1) of the empty block empties[first + (t >> LOG_PXB)], if the list reaches that far.  The
// thread adds that value T times to the pixel's running sum -- the additions sum_block() would perform on the parked values,
// in the same order -- and traces nothing.  One device atomic per workgroup: the segments of its blocks' pixels in the frame.
template <int OUTPUT> BT_DEV void fill_empty_blocks(const BtLaunch &P, const uint32_t *empties, uint32_t first, uint32_t n_empty) {
    const BlockGeom G = block_geom(P);
    const uint32_t T = (uint32_t)P.samples * (uint32_t)(P.subsample_n * P.subsample_n);
    V3 value;
    if (OUTPUT == 0) {
        value = mk(0, 0, 0) + mk(1, 1, 1) * mk(P.root_color);      // L = L + beta * root_color, fresh L and beta
    } else if (OUTPUT == 1) {
        value = mk(P.root_albedo);
    } else {
        const float fd = P.root_has_albedo ? P.clip_max : __builtin_inff();
        float depth = (fd - P.clip_min) / (P.clip_max - P.clip_min);
        depth = fminf(fmaxf(depth, 0.0f), 1.0f);
        value = mk(depth, depth, depth);
    }
    const uint32_t e = first + (threadIdx.x >> G.LOG_PXB);
    if (e < n_empty) {
        const BlockRef B = block_ref(P, G, empties[e]);
        const PixelRef r = pixel_of(P, G, B, threadIdx.x & (G.pxb - 1u));
        if (r.in_frame) {
            float *o = out_of(P, P.out, B, r);
            V3 sum = mk(o[0], o[1], o[2]);
            for (uint32_t k = 0; k < T; ++k) sum = sum + value;
            o[0] = sum.x;
            o[1] = sum.y;
            o[2] = sum.z;
        }
    }
    if (P.counters && threadIdx.x < 64u) {         // the first wave: lane j counts the pixels of the workgroup's j-th block
        uint32_t pixels = 0;
        if (threadIdx.x < G.NS && first + threadIdx.x < n_empty) {
            const BlockRef B = block_ref(P, G, empties[first + threadIdx.x]);
            uint32_t nx = 0, ny = 0;
            block_extent(P, G, B, nx, ny);
            pixels = nx * ny;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) pixels += __shfl_xor(pixels, off, 64);
        if (threadIdx.x == 0 && pixels != 0u) atomicAdd(&P.counters[0], (unsigned long long)pixels * T);
    }
}

// the inclusive prefix sum of `v` over the lanes of a wave
BT_DEV uint32_t wave_scan_incl(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(v, off, 64);
        if ((int)lane >= off) v += o;
    }
    return v;
}

} // namespace

// One thread per pixel block of a launch: masks[b] = btcull::block_mask (bt_cull.hpp), the rows read through the constant
// address space.  Microseconds of double-precision work per camera; bt_api.cpp keeps the result on the scene handle.
__global__ __launch_bounds__(256) void bt_block_mask_kernel(BtLaunch P, uint32_t n_blocks, unsigned long long *masks) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    typedef const __attribute__((address_space(4))) BtSphereRow RowK;
    masks[b] = btcull::block_mask(P, (RowK *)P.sphere_rows, b);
}

// The blocks of a launch in the order the CULL builds of the render kernel take them: out = {n_live, n_empty, order[n_blocks]},
// word for word what btcull::block_order (bt_cull.hpp) writes.  ONE workgroup, launched behind bt_block_mask_kernel on the same
// stream (stream order is all the ordering there is): it counts the non-zero masks, then scans them in chunks of
// BT_ORDER_CHUNK -- four consecutive masks per thread, a wave scan, the 16 wave totals through LDS (two sets, alternating:
// one barrier per chunk).  Once per camera, like the masks.
#define BT_ORDER_THREADS 1024
#define BT_ORDER_PER_THREAD 4
#define BT_ORDER_CHUNK (BT_ORDER_THREADS * BT_ORDER_PER_THREAD)
__global__ __launch_bounds__(BT_ORDER_THREADS) void bt_block_order_kernel(const unsigned long long *masks, uint32_t n_blocks, uint32_t *out) {
    constexpr uint32_t NW = BT_ORDER_THREADS / 64;
    __shared__ uint32_t s_wave[2][NW];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t mine = 0;
    for (uint32_t b = t; b < n_blocks; b += BT_ORDER_THREADS) mine += masks[b] != 0ull ? 1u : 0u;
    uint32_t incl = wave_scan_incl(mine, lane);
    if (lane == 63u) s_wave[0][wave] = incl;
    __syncthreads();
    uint32_t n_live = 0;
    for (uint32_t w = 0; w < NW; ++w) n_live += s_wave[0][w];
    if (t == 0) {
        out[0] = n_live;
        out[1] = n_blocks - n_live;
    }
    uint32_t *order = out + BT_ORDER_HEADER;
    uint32_t live_base = 0, set = 1;               // live blocks ahead of this chunk
    for (uint32_t c0 = 0; c0 < n_blocks; c0 += BT_ORDER_CHUNK, set ^= 1u) {
        const uint32_t b0 = c0 + t * BT_ORDER_PER_THREAD;
        bool live[BT_ORDER_PER_THREAD];
        mine = 0;
#pragma unroll
        for (uint32_t j = 0; j < BT_ORDER_PER_THREAD; ++j) {
            live[j] = b0 + j < n_blocks && masks[b0 + j] != 0ull;
            mine += live[j] ? 1u : 0u;
        }
        incl = wave_scan_incl(mine, lane);
        if (lane == 63u) s_wave[set][wave] = incl;
        __syncthreads();
        uint32_t before = live_base + incl - mine, total = 0;      // live blocks ahead of b0
        for (uint32_t w = 0; w < NW; ++w) {
            const uint32_t v = s_wave[set][w];
            total += v;
            if (w < wave) before += v;
        }
#pragma unroll
        for (uint32_t j = 0; j < BT_ORDER_PER_THREAD; ++j) {
            const uint32_t b = b0 + j;
            if (b >= n_blocks) break;
            if (live[j]) order[before++] = b;
            else order[n_live + (b - before)] = b;                 // b - before: empty blocks ahead of b
        }
        live_base += total;
    }
}

// --------------------------------------------------------------------------------------------
// The render kernel.  OUTPUT: 0 Full, 1 Albedo, 2 Normal, 3 Depth (tracer/mod.rs:108-115); 4 = Full plus the three others
// from the same paths, each into a frame of its own (guided render, an EXTENSION: bt_render_guided_device);
// 5 = Full into the tiles that BtLaunch::tile_active marks, plus each pixel's second moment (adaptive sampling, an EXTENSION:
// bt_render_adaptive_device; LENS = PACKED = false only).
// Block = 256 threads; 7 waves per SIMD caps the allocation at 72 VGPRs (round 2, without the SLP vectorizer;
// profiles/r03c/ab_waves_noslp.log, ab_waves_per_class.log).
#ifndef BT_WAVES_PER_SIMD
#define BT_WAVES_PER_SIMD 7
#endif
#ifndef BT_WAVES_PER_SIMD_VOLS
#define BT_WAVES_PER_SIMD_VOLS BT_WAVES_PER_SIMD     // sphere scenes with volumes (own knob for A/B runs)
#endif
#ifndef BT_WAVES_PER_SIMD_RECTS
#define BT_WAVES_PER_SIMD_RECTS 7
#endif
#ifndef BT_WAVES_PER_SIMD_LENS
#define BT_WAVES_PER_SIMD_LENS 6       // lens builds: 80 VGPRs + ~100 B of scratch per lane still beat 4 waves without
#endif                                 // scratch (665 -> 719 Msamples/s, profiles/r01g/ab_lens_waves.log)
#ifndef BT_WAVES_PER_SIMD_GUIDED_RECTS
#define BT_WAVES_PER_SIMD_GUIDED_RECTS 7   // guided (OUTPUT == 4) rect builds without volumes: own knob for A/B runs
#endif
#ifndef BT_SGPR_DIET
#define BT_SGPR_DIET 1         // sphere-only builds without volumes: wave-uniform values out of the SGPR file, kernels under an SGPR
#endif                         // budget of their own; 0 = the form and the kernels of the other builds, for A/B runs
#ifndef BT_WAVES_PER_SIMD_DIET
#define BT_WAVES_PER_SIMD_DIET BT_WAVES_PER_SIMD     // ... their register-allocation target (they use 54 ... 58 VGPRs: eight waves fit) ...
#endif
#ifndef BT_DIET_NUM_SGPR
#define BT_DIET_NUM_SGPR 80    // ... and their SGPR budget: the granule that admits an eighth workgroup per CU (96: seven)
#endif
// LENS switches the (non-reference, default-off) gravitational-lens extension of bt_device.hpp in.
#ifndef BT_SKIP_DIR
#define BT_SKIP_DIR 1          // a wave of pass-through march steps skips the direction sampling
#endif
#ifndef BT_LENS_BATCH
#define BT_LENS_BATCH 8            // RK4 steps a lane marches per loop iteration before it yields
#endif
// RECTS = false: sphere-only scenes (scene.json, volume.json, cloud.json) run a build without any rect / cuboid code.
// VOLS = false: no sphere carries a volume (scene.json, the Cornell boxes): the march and Volume::shade drop out.
// PACKED = true: the builds for packed launches (BtLaunch::wg_blocks > 1; not with the lens extension), so that the
// other builds carry none of their code -- as a run-time switch it cost C3 4 % (profiles/r04u).
template <int OUTPUT, bool LENS, bool RECTS, bool VOLS, bool PACKED>
__global__ __launch_bounds__(256, (OUTPUT == 4 && RECTS && !VOLS) ? BT_WAVES_PER_SIMD_GUIDED_RECTS : LENS ? BT_WAVES_PER_SIMD_LENS : (RECTS ? BT_WAVES_PER_SIMD_RECTS : (VOLS ? BT_WAVES_PER_SIMD_VOLS : BT_WAVES_PER_SIMD))) void bt_render_kernel(BtLaunch P) {
#include "bt_render_body.inc"
}
// The sphere-only builds without volumes, lens or packing (outputs 0 ... 3): the same body as kernels with an SGPR budget of
// their own.  A CU admits 256-thread workgroups by SGPR granule: eight up to 80 SGPRs, seven from 82 to 96 -- whatever the
// compiler's occupancy line and the occupancy API say (tools/residency_census.hip, profiles/r15/census.txt).  With the body's
// DIET forms these builds fit 80 with fewer spills than they had at 96 (tests/test_kernel_resources.py), and the eighth
// workgroup then pays (profiles/r15).  amdgpu_num_sgpr takes no template argument, hence explicit specialisations.
#if BT_SGPR_DIET
template <> __global__ __launch_bounds__(256, BT_WAVES_PER_SIMD_DIET) __attribute__((amdgpu_num_sgpr(BT_DIET_NUM_SGPR)))
void bt_render_kernel<0, false, false, false, false>(BtLaunch P) {
    constexpr int OUTPUT = 0;
    constexpr bool LENS = false, RECTS = false, VOLS = false, PACKED = false;
#include "bt_render_body.inc"
}
template <> __global__ __launch_bounds__(256, BT_WAVES_PER_SIMD_DIET) __attribute__((amdgpu_num_sgpr(BT_DIET_NUM_SGPR)))
void bt_render_kernel<1, false, false, false, false>(BtLaunch P) {
    constexpr int OUTPUT = 1;
    constexpr bool LENS = false, RECTS = false, VOLS = false, PACKED = false;
#include "bt_render_body.inc"
}
template <> __global__ __launch_bounds__(256, BT_WAVES_PER_SIMD_DIET) __attribute__((amdgpu_num_sgpr(BT_DIET_NUM_SGPR)))
void bt_render_kernel<2, false, false, false, false>(BtLaunch P) {
    constexpr int OUTPUT = 2;
    constexpr bool LENS = false, RECTS = false, VOLS = false, PACKED = false;
#include "bt_render_body.inc"
}
template <> __global__ __launch_bounds__(256, BT_WAVES_PER_SIMD_DIET) __attribute__((amdgpu_num_sgpr(BT_DIET_NUM_SGPR)))
void bt_render_kernel<3, false, false, false, false>(BtLaunch P) {
    constexpr int OUTPUT = 3;
    constexpr bool LENS = false, RECTS = false, VOLS = false, PACKED = false;
#include "bt_render_body.inc"
}
#endif

// shard (tile-major, `world` ranks back to back) -> row-major frame; rgb AND alpha copied.
__global__ __launch_bounds__(256) void bt_unshard_kernel(const float4 *gathered, float4 *frame, uint32_t width,
                                                         uint32_t height, uint32_t tiles_x, uint32_t tiles_y,
                                                         uint32_t world, uint32_t tiles_per_rank) {
    const uint32_t tile = blockIdx.x;
    if (tile >= tiles_x * tiles_y) return;
    const uint32_t rank = tile % world, slot = tile / world;
    const uint32_t lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const uint32_t px = (tile % tiles_x) * BT_TILE_DIM + lx, py = (tile / tiles_x) * BT_TILE_DIM + ly;
    if (px >= width || py >= height) return;
    const size_t src = ((size_t)rank * tiles_per_rank + slot) * (BT_TILE_DIM * BT_TILE_DIM) + ly * BT_TILE_DIM + lx;
    frame[(size_t)py * width + px] = gathered[src];
}

// Buffer::preview (buffer.rs:117-138): mean -> colour space -> (x * 255) as u8.
__global__ __launch_bounds__(256) void bt_preview_kernel(const float4 *rgba, uint32_t *out, uint32_t n,
                                                         float samples_recip, int color_space) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 s = rgba[i];
    V3 rgb = mk(s.x, s.y, s.z) * samples_recip;
    if (color_space == 1) {
        V3 nrm = normalize(rgb);
        rgb = (nrm + mk(1, 1, 1)) * 0.5f;
    } else if (color_space == 3) {
        rgb = mk(linear_to_srgb(rgb.x), linear_to_srgb(rgb.y), linear_to_srgb(rgb.z));
    }
    out[i] = f32_to_u8(rgb.x) | (f32_to_u8(rgb.y) << 8) | (f32_to_u8(rgb.z) << 16) | (f32_to_u8(s.w) << 24);
}

// bt_debug_philox_device (tests): philox_ukeys() -- the call of the sphere-only render builds -- over caller-given (counter, key)
// pairs.  Lane l of a wave holds pair 64 * wave + l; the wave goes through its 64 keys one at a time (readlane: wave-uniform, as
// a launch's seed is), every lane runs its own counter under that key and keeps the result of its own turn.
__global__ __launch_bounds__(256) void bt_philox_test_kernel(const uint32_t *pairs, uint32_t n, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t *q = pairs + 6 * (size_t)(i < n ? i : n - 1u);
    const uint32_t c0 = q[0], c1 = q[1], c2 = q[2], c3 = q[3], k0 = q[4], k1 = q[5];
    U4 mine = {0u, 0u, 0u, 0u};
    for (int j = 0; j < 64; ++j) {
        const uint32_t kj0 = (uint32_t)__builtin_amdgcn_readlane((int)k0, j), kj1 = (uint32_t)__builtin_amdgcn_readlane((int)k1, j);
        const U4 u = philox_ukeys(c0, c1, c2, c3, kj0, kj1);
        if ((int)(threadIdx.x & 63u) == j) mine = u;
    }
    if (i < n) {
        out[4 * (size_t)i + 0] = mine.x; out[4 * (size_t)i + 1] = mine.y;
        out[4 * (size_t)i + 2] = mine.z; out[4 * (size_t)i + 3] = mine.w;
    }
}

// ---- host-side launchers (called from bt_api.cpp) ---------------------------------------------
// bt_debug_primary_mask: the masks bt_block_mask_kernel writes, one per block of the launch `P` describes (blocks in launch
// order), bit i = sphere row i may be hit; computed here on the host by the same function (bt_cull.hpp block_mask).
extern "C" void bt_primary_masks_host(const BtLaunch *P, const BtSphereRow *rows, uint32_t n_blocks, uint64_t *out) {
    for (uint32_t b = 0; b < n_blocks; ++b) out[b] = btcull::block_mask(*P, rows, b);
}
// Does a launch of `P` run a build that reads BtLaunch::block_masks / block_order (the kernel's CULL)?
extern "C" int bt_launch_reads_masks(const BtLaunch *P, int output) {
    return !P->any_rects && !P->any_volumes && !P->lens_on && P->wg_blocks <= 1 && output != 2 && output != 4 && output != 5 && P->max_bounces >= 0;
}
// 1: bt_api.cpp may keep a launch's masks on the scene handle; 0 (A/B variant -DBT_MASK_NOCACHE): every render computes them
extern "C" int bt_mask_cache_enabled(void) {
#ifdef BT_MASK_NOCACHE
    return 0;
#else
    return 1;
#endif
}
extern "C" hipError_t bt_launch_block_masks(const BtLaunch *P, uint32_t n_blocks, uint64_t *masks, hipStream_t stream) {
    if (n_blocks == 0 || !masks || (P->n_prims > 0 && !P->sphere_rows)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bt_block_mask_kernel, dim3((n_blocks + 255u) / 256u), dim3(256), 0, stream, *P, n_blocks,
                       (unsigned long long *)masks);
    return hipGetLastError();
}
// btcull::block_order's words ({n_live, n_empty, order[n_blocks]}) on the device, from the masks bt_launch_block_masks has written on the same stream
extern "C" hipError_t bt_launch_block_order(const uint64_t *masks, uint32_t n_blocks, uint32_t *out, hipStream_t stream) {
    if (n_blocks == 0 || !masks || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bt_block_order_kernel, dim3(1), dim3(BT_ORDER_THREADS), 0, stream, (const unsigned long long *)masks,
                       n_blocks, out);
    return hipGetLastError();
}
extern "C" hipError_t bt_launch_philox_test(const uint32_t *pairs, uint32_t n, uint32_t *out, hipStream_t stream) {
    if (n == 0 || !pairs || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bt_philox_test_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, pairs, n, out);
    return hipGetLastError();
}
extern "C" hipError_t bt_launch_render(const BtLaunch *P, int output, unsigned grid, size_t lds_bytes,
                                       hipStream_t stream) {
    // grid = tiles to render; a tile is P->slices workgroups (see the mapping in the kernel)
    const bool packed = P->wg_blocks > 1;          // bt_api.cpp packs launches without the lens only
    if (packed && P->lens_on) return hipErrorInvalidValue;
    if (bt_launch_reads_masks(P, output) && (!P->block_masks || !P->block_order)) return hipErrorInvalidValue;   // no masks or no order, no launch
    dim3 g(packed ? P->n_workgroups : grid * (unsigned)P->slices), b(256);
    // scene classes: bit 0 = some sphere carries a volume (volume.json, cloud.json), bit 1 = rects / cuboids present
    // (the Cornell boxes); scene.json is class 0
    const int cls = (P->any_rects ? 2 : 0) | (P->any_volumes ? 1 : 0);
    // scene tables beyond the default 64 KB of dynamic LDS (hundreds of objects): gfx950 has 160 KB per CU, the limit
    // has to be raised per kernel; one workgroup per CU is then all that fits
#define BT_LAUNCH(O, L, R, V, K)                                                                                 \
    do {                                                                                                         \
        if (lds_bytes > 48 * 1024)                                                                               \
            (void)hipFuncSetAttribute((const void *)bt_render_kernel<O, L, R, V, K>,                             \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);               \
        hipLaunchKernelGGL((bt_render_kernel<O, L, R, V, K>), g, b, lds_bytes, stream, *P);                      \
    } while (0)
#define BT_LAUNCH_OUT(L, R, V, K)                                                                                \
    switch (output) {                                                                                            \
    case 0: BT_LAUNCH(0, L, R, V, K); break;                                                                     \
    case 1: BT_LAUNCH(1, L, R, V, K); break;                                                                     \
    case 2: BT_LAUNCH(2, L, R, V, K); break;                                                                     \
    default: BT_LAUNCH(3, L, R, V, K); break;                                                                    \
    }
#define BT_LAUNCH_CLASS(L, K)                                                                                    \
    if (cls == 3) { BT_LAUNCH_OUT(L, true, true, K) } else if (cls == 2) { BT_LAUNCH_OUT(L, true, false, K) }      \
    else if (cls == 1) { BT_LAUNCH_OUT(L, false, true, K) } else { BT_LAUNCH_OUT(L, false, false, K) }
    if (output == 5) {                             // adaptive pass (extension): four builds, neither lens nor packed
        if (P->lens_on || packed || !P->tile_active || !P->moment) return hipErrorInvalidValue;
        if (cls == 3) BT_LAUNCH(5, false, true, true, false); else if (cls == 2) BT_LAUNCH(5, false, true, false, false);
        else if (cls == 1) BT_LAUNCH(5, false, false, true, false); else BT_LAUNCH(5, false, false, false, false);
    } else if (output == 4) {                      // guided render (extension): no lens builds
        if (P->lens_on) return hipErrorInvalidValue;
#define BT_LAUNCH_GUIDED(K)                                                                                      \
        if (cls == 3) BT_LAUNCH(4, false, true, true, K); else if (cls == 2) BT_LAUNCH(4, false, true, false, K);    \
        else if (cls == 1) BT_LAUNCH(4, false, false, true, K); else BT_LAUNCH(4, false, false, false, K);
        if (packed) { BT_LAUNCH_GUIDED(true) } else { BT_LAUNCH_GUIDED(false) }
#undef BT_LAUNCH_GUIDED
    } else if (packed) {
        BT_LAUNCH_CLASS(false, true)
    } else if (P->lens_on) {
        BT_LAUNCH_CLASS(true, false)
    } else {
        BT_LAUNCH_CLASS(false, false)
    }
#undef BT_LAUNCH_CLASS
#undef BT_LAUNCH_OUT
#undef BT_LAUNCH
    return hipGetLastError();
}
extern "C" hipError_t bt_launch_unshard(const float *gathered, float *frame, uint32_t width, uint32_t height,
                                        uint32_t tiles_x, uint32_t tiles_y, uint32_t world, uint32_t tiles_per_rank,
                                        hipStream_t stream) {
    hipLaunchKernelGGL(bt_unshard_kernel, dim3(tiles_x * tiles_y), dim3(256), 0, stream, (const float4 *)gathered,
                       (float4 *)frame, width, height, tiles_x, tiles_y, world, tiles_per_rank);
    return hipGetLastError();
}
extern "C" hipError_t bt_launch_preview(const float *rgba, uint8_t *out, uint32_t n, uint32_t samples,
                                        int color_space, hipStream_t stream) {
    float recip = 1.0f / (float)samples;
    hipLaunchKernelGGL(bt_preview_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const float4 *)rgba,
                       (uint32_t *)out, n, recip, color_space);
    return hipGetLastError();
}
