// bt_plan.hpp -- the shape of a render's launches: every number bt_api.cpp's render_common needs before it
// touches the device -- samples per launch, slices, the packed launch and its LDS record pool, the LDS budget, where the
// guides' planes lie in the scratch -- decided from the filled BtLaunch, the flat scene, bt_tuning and the GPU's CU count.
//
// Nothing here calls HIP.  Device memory comes in through one callback (reserve_scratch's `realloc`): render_common hands in
// hipStreamSynchronize / hipFree / hipMalloc, bt_debug_plan_launch a byte limit, so tests/test_launch_plan.py runs the
// planner -- the allocation-failure branches included -- on a machine without a GPU.  None of these shapes can change a pixel
// (bt_tuning), so only tests that look at the shape itself (bt_stats) can see a slip here.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/bendy_hip.h"
#include "bt_scene.hpp"
#include "bt_types.h"

#ifndef BT_POOL_RECORDS
#define BT_POOL_RECORDS 128        // PathRec records per workgroup for the drain of a packed rect launch (at most 256)
#endif

static_assert(BT_TILE == BT_TILE_DIM, "public and device tile sizes must agree");

namespace btplan {

constexpr uint64_t kDefaultScratchCap = 2ull << 30;   // parked sample values per launch; deeper renders are split
constexpr uint32_t kScratchShrinkAfter = 8;           // renders in a row that need < 1/4 of the scratch before it shrinks

// ---- tiles of a frame ------------------------------------------------------------------------------------------------
// The frame is cut into BT_TILE x BT_TILE tiles, numbered row-major; rank r of `world` owns tiles r, r + world, ...
inline uint32_t tiles_across(uint32_t extent) { return (extent + BT_TILE - 1) / BT_TILE; }
inline uint32_t frame_tiles(uint32_t width, uint32_t height) { return tiles_across(width) * tiles_across(height); }
inline uint32_t tiles_per_rank(uint32_t n_tiles, uint32_t world) { return (n_tiles + world - 1) / world; }
// pixels inside the frame of rank `rank`'s tiles, each tile's counted `weight[tile]` times (null: once)
inline uint64_t pixels_owned(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, const uint32_t *weight = nullptr) {
    const uint32_t tiles_x = tiles_across(width), n_tiles = frame_tiles(width, height);
    uint64_t pixels = 0;
    for (uint32_t t = rank; t < n_tiles; t += world) {
        const uint32_t tx = t % tiles_x, ty = t / tiles_x;
        const uint32_t w = std::min<uint32_t>(BT_TILE, width - tx * BT_TILE), h = std::min<uint32_t>(BT_TILE, height - ty * BT_TILE);
        pixels += (uint64_t)w * h * (weight ? weight[t] : 1u);
    }
    return pixels;
}
// Which tiles a launch of `P` renders; returns its grid (tiles).  sharded: this rank's tiles only, into its shard.
inline uint32_t shard_launch(BtLaunch &P, uint32_t rank, uint32_t world, bool sharded) {
    P.rank = rank;
    P.world = world;
    P.sharded = sharded ? 1 : 0;
    const uint32_t n_tiles = P.tiles_x * P.tiles_y;
    return sharded ? tiles_per_rank(n_tiles, world) : n_tiles;
}

inline bool any_prim_carries_volume(const std::vector<BtPrim> &prims) {
    for (const BtPrim &R : prims)
        if (R.volume >= 0) return true;
    return false;
}

// ---- the scratch a handle keeps between renders ------------------------------------------------------------------------
struct Scratch {
    uint64_t bytes = 0;            // held
    uint32_t small_streak = 0;     // consecutive renders that needed less than a quarter of the scratch held
};
// Does the scratch held serve a render that needs `need` bytes?  false: free it and allocate `need` bytes.
inline bool scratch_serves(Scratch &held, uint64_t need) {
    // Grow when too small.  Give memory back only after kScratchShrinkAfter consecutive renders that each needed less
    // than a quarter of what is held: a caller that alternates deep renders with shallow previews on one handle keeps
    // its scratch (no hipFree / hipMalloc -- a device-wide synchronisation -- per call); bt_scene_trim() returns it at once.
    if (held.bytes >= need) {
        if (held.bytes / 4 <= need) { held.small_streak = 0; return true; }
        if (++held.small_streak < kScratchShrinkAfter) return true;
    }
    held.small_streak = 0;
    return false;
}
// `realloc(need)` frees what is held, allocates `need` bytes (nothing for 0) and returns the bytes held afterwards.
template <class Realloc> bool reserve_scratch(Scratch &held, uint64_t need, Realloc &&realloc) {
    if (scratch_serves(held, need)) return true;
    held.bytes = realloc(need);
    return held.bytes == need;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------
// The kind of pass (bt_api.cpp RenderPass).  GUIDED with no guide present is the Full render, build and all.
enum { PLAIN = 0, GUIDED = 1, ADAPTIVE = 2 };

struct Plan {
    int output = 0;                // the build: the Output mode, 4 = guided, 5 = adaptive
    uint32_t grid = 0;             // tiles of a launch
    uint32_t chunk = 0;            // samples per launch
    uint32_t launches = 0;
    size_t lds_bytes = 0;          // dynamic LDS of a workgroup
    uint64_t guide_values[3] = {}; // guided: floats from the scratch's start to each guide's plane (0 = guide absent)
    uint64_t parked_bytes = 0;     // bt_stats.parked_bytes
    uint64_t pixels = 0;           // pixels this rank owns
    std::string error;             // what a non-zero return of plan_launch is about
};

// Shape of the launch.  A workgroup owns a block of 256 / S pixels and deals their samples to its lanes,
// every sample's value is parked in `scratch` (12 B per sample of the launch).  S is chosen so that a workgroup holds
// ~16 samples per lane (4 with the lens on, whose paths differ far more in length; down to 4 as well when the launch has
// too few pixels to fill the GPU).  A render whose scratch would exceed the cap is issued as several launches over
// consecutive sample ranges (k launches of m samples == one launch of k * m samples).  bt_tuning
// (bt_scene_set_tuning) pins any of these for tests and A/B tools.
//
// `P`: fill_launch's, with shard_launch applied; the shape fields are written into it (not `scratch` and the guides'
// planes, which are pointers: Plan::guide_values).  `output`: the effective Output mode.  `guides`: bit g = guide g is present.
// Returns 0, or a bt_status with Plan::error set.
template <class Realloc>
int plan_launch(BtLaunch &P, int output, const bt::FlatScene &flat, const bt_tuning &tune, uint32_t n_cu, int kind, uint32_t guides,
                Scratch &held, Realloc &&realloc, Plan &plan) {
    // Guided render: the OUTPUT == 4 builds park 12 more bytes per sample for the albedo, 12 for the normal and 4 for the depth,
    // each only if its frame is given.  Without any guide it is the Full render, build and all.
    const bool guided = kind == GUIDED && (guides & 7u) != 0, adapt = kind == ADAPTIVE;
    uint64_t sample_bytes = 3 * sizeof(float);                            // bytes parked per sample: 12 for the colour value
    if (guided) {
        output = 4;
        for (int g = 0; g < 3; ++g)
            if (guides >> g & 1u) sample_bytes += (g == 2 ? 1 : 3) * sizeof(float);
    }
    if (adapt) output = 5;                                                // (the OUTPUT == 5 builds, never packed)
    plan.output = output;
    const uint32_t grid = P.sharded ? tiles_per_rank(P.tiles_x * P.tiles_y, P.world) : P.tiles_x * P.tiles_y;
    plan.grid = grid;

    const uint32_t nn = (uint32_t)(P.subsample_n * P.subsample_n);
    const uint64_t px_launch = (uint64_t)grid * BT_TILE_DIM * BT_TILE_DIM;
    uint32_t chunk = (uint32_t)P.samples;                         // samples per launch
    P.slices = 1;
    P.table_lds_bytes = (uint32_t)flat.lds_bytes();
    size_t lds_bytes = flat.lds_bytes();
    {
        // scenes with volumes: the BtVolBox table behind the scene tables; density maps whose bounds tests cannot fire
        bool safe = true;
        for (const BtVolume &v : flat.volumes)
            safe = safe && v.width >= 1 && v.height >= 1 && v.depth >= 1 && v.size.x >= 0.0f && v.size.y >= 0.0f && v.size.z >= 0.0f &&
                   std::ceil(v.size.x) <= (float)(v.width - 1) && std::ceil(v.size.y) <= (float)(v.height - 1) &&
                   std::ceil(v.size.z) <= (float)(v.depth - 1);
        safe = safe && flat.density.size() < (1u << 24);         // density_sample_safe() indexes with 24-bit multiply-adds
        P.vols_safe = safe ? 1 : 0;
        P.vbox_lds_bytes = any_prim_carries_volume(flat.prims) ? (uint32_t)(sizeof(BtVolBox) * flat.prims.size()) : 0u;
        if (lds_bytes + P.vbox_lds_bytes > 32 * 1024) P.vbox_lds_bytes = 0;          // big scenes keep the per-step arithmetic
        lds_bytes += P.vbox_lds_bytes;
    }
#ifdef BT_LDS_PAD                                   // developer build: unused LDS per workgroup, to time lower occupancies
    lds_bytes += BT_LDS_PAD;
#endif
    // the launch should hold >= 4 x 20 waves per CU (tuned on the MI355X's 256 CUs as "4 * 5120 waves", round 1d)
    const uint64_t wave_slots = (uint64_t)n_cu * 20;
    const uint64_t T_all = (uint64_t)P.samples * nn;
    const uint64_t per_sample = px_launch * nn * sample_bytes;               // 12 B per parked sample value (+ the guides')
    const uint64_t cap = tune.scratch_cap_bytes ? tune.scratch_cap_bytes : kDefaultScratchCap;
    if (per_sample * chunk > cap) chunk = (uint32_t)std::max<uint64_t>(1, cap / per_sample);
    // the parked values need device memory; when it cannot be had, render fewer samples per launch (there is no path that
    // does without: a lane that owned a pixel and summed in a register lost every measurement and left in round 3)
    while (!reserve_scratch(held, per_sample * chunk, realloc)) {
        if (chunk == 1) {
            plan.error = "no device memory for the parked samples (" + std::to_string(per_sample) + " bytes per sample)";
            return BT_ERR_DEVICE;
        }
        chunk = (chunk + 1) / 2;
    }
    auto pick = [&](uint64_t T) -> uint32_t {
        if (tune.slices) return tune.slices;
        uint32_t S = 1;
        if (P.lens_on) {
            while (S < 32 && T / (2 * S) >= 4) S *= 2;       // lens paths differ far more in length: ~4 samples per lane
        } else {
            // Measured on 1080p and 512 x 512 frames, T = 1 ... 128 rays per pixel per launch, and on the shards of 2 / 4 / 8
            // ranks with 128 / 256 / 512 rays (profiles/r02z/time_shallow_before.log, time_shallow_512_before.log, time_shard.log).
            // A launch wants ~21 rounds of workgroups over the GPU (tiles x S ~ 32 000 on 256 CUs: S = 4 for a full 1080p
            // frame, 8 / 16 / 32 for the shards) with >= 8 samples per lane; below half of that, 4 samples per lane are
            // enough; and a frame that cannot even fill the wave slots twice is cut down to one sample per lane.
            const uint64_t target = 21ull * (uint64_t)n_cu * 6;
            while (S < 32 && (uint64_t)grid * (2 * S) * 4 <= 5 * target && T / (2 * S) >= 8) S *= 2;
            while (S < 32 && (uint64_t)grid * S * 2 < target && T / (2 * S) >= 4) S *= 2;
            while (S < 32 && (uint64_t)grid * 4 * S < 2 * wave_slots && T / (2 * S) >= 1) S *= 2;
            // Sphere-only scenes (cheaper items, eight waves per SIMD) want more, smaller workgroups on small frames than the rect
            // builds: up to ~7 500 of them while a lane still gets a whole item (profiles/r04j: scene.json 768 x 512 with the
            // reference CLI's 1 sample x Subpixel(2): S = 2 -> 4, 0.129 -> 0.119 ms; 8 rays: 0.197 -> 0.167; 1280 x 720 x 4:
            // 0.212 -> 0.184; the Cornell boxes lose with the same change)
            if (!P.any_rects)
                while (S < 32 && (uint64_t)grid * (2 * S) <= 30ull * (uint64_t)n_cu && 256 * T / (2 * S) >= 256) S *= 2;
        }
        return S;
    };
    P.slices = (int32_t)pick((uint64_t)chunk * nn);
    // a workgroup counts its path segments in 32 bits (bt_stats.segments): keep its work items x the longest possible path
    // below 2^32 -- only a pinned launch shape (bt_tuning.slices with an enormous scratch cap) can get near
    const uint64_t longest = ((uint64_t)P.max_bounces + 2) * ((uint64_t)P.max_volume_bounces + 3) + (P.lens_on ? 2 : 0);
    const uint64_t items_max = std::max<uint64_t>(1, 0xffffffffull / longest);
    {
        const uint64_t pxb = 256u / (uint32_t)P.slices;
        if (pxb * chunk * nn > items_max) chunk = (uint32_t)std::max<uint64_t>(1, items_max / (pxb * nn));
    }
    // Packed launch: when the whole render is one launch of at most a few generations of workgroups, ONE generation -- a workgroup
    // per workgroup slot of the GPU, each owning every n_workgroups-th small pixel block behind one queue -- ends with one drain
    // of its longest paths instead of one per generation.
    P.wg_blocks = 1;
    P.wg_blocks_rem = 0;
    P.n_workgroups = 0;
    P.log_rows = 0;
    P.row_mask = 0xffffffffu;
    P.pool_records = 0;
    P.pool_lds_offset = 0;
    // The drain of a packed launch compacts the paths in flight through LDS records (bt_kernels.hip PathRec, 80 B): room for 128
    // behind the tables, where that does not cost a workgroup slot and the packed record fields are wide enough.
    const size_t pool_offset = (lds_bytes + 15) & ~(size_t)15, pool_bytes = BT_POOL_RECORDS * 80;
    bool pool_ok = tune.packed != 1 && P.any_rects && !P.any_volumes && output == 0 &&   // (the Full-output rect build is the one that has the code)
                   P.max_bounces < 0xfff0 && P.max_volume_bounces < 0xfff0 && flat.prims.size() < 0xfffff0u;
    // workgroup slots of the GPU: 7 per CU by the builds' __launch_bounds__ (72 VGPRs), fewer when the scene tables are large
    // (160 KB of LDS per CU, allocated in 2 KB steps here to stay on the safe side)
    auto slots_per_cu = [](size_t lds) { return std::max(1u, std::min(7u, 160u * 1024u / (uint32_t)((lds + 64 + 2047) & ~(size_t)2047))); };
    pool_ok = pool_ok && slots_per_cu(pool_offset + pool_bytes) == slots_per_cu(lds_bytes);
    const uint32_t wg_slots = n_cu * slots_per_cu(lds_bytes);
    const uint64_t T_launch = (uint64_t)chunk * nn;
    uint64_t values = px_launch * T_launch;                      // sample values a launch parks: one per work item
    // Measured (profiles/r04t: 256 x 256 ... 1920 x 1080 frames, 1 ... 64 rays per pixel, three scene classes): packing pays
    // between ~1 and ~24 work items per lane of the GPU (scene.json 768 x 512 x 4: 0.121 -> 0.09 ms); deeper launches overlap
    // their drains with other workgroups' work and lose 5 - 20 % when packed, emptier ones do not fill the slots
    const uint64_t items_all = px_launch * T_launch, lanes_all = (uint64_t)wg_slots * 256;
    const bool pack = tune.packed > 0 || (tune.packed < 0 && items_all > lanes_all && items_all <= 24 * lanes_all);
    if (pack && chunk == (uint32_t)P.samples && !P.lens_on && !adapt) {           // (the lens extension and the adaptive pass have no packed builds)
        // blocks of ~64 / T pixels: one wave's take from the queue is one block's samples (coherent camera rays)
        uint32_t S = 4;
        while (S < 32 && S < 4 * T_launch) S *= 2;
        if (tune.slices) S = tune.slices;
        const uint64_t blocks = (uint64_t)grid * S, per_wg = (blocks + wg_slots - 1) / wg_slots;
        uint32_t log_rows = 0;                                   // T padded to a power of two: rows of a block in the queue
        while ((1ull << log_rows) < T_launch) log_rows += 1;
        const uint64_t wg_items = (per_wg * (256u / S)) << log_rows;
        const uint64_t need = (uint64_t)wg_slots * wg_items * sample_bytes;
        if (blocks > wg_slots && blocks <= 0x7fffffffu && wg_items <= items_max &&
            (need <= held.bytes || reserve_scratch(held, need, realloc))) {
            P.slices = (int32_t)S;
            P.n_workgroups = wg_slots;
            P.wg_blocks = (uint32_t)per_wg;
            P.wg_blocks_rem = (uint32_t)(blocks - (per_wg - 1) * wg_slots);
            P.log_rows = log_rows;
            P.row_mask = (1u << log_rows) - 1u;
            values = (uint64_t)wg_slots * wg_items;
            if (pool_ok) {
                P.pool_records = BT_POOL_RECORDS;
                P.pool_lds_offset = (uint32_t)pool_offset;
                lds_bytes = pool_offset + pool_bytes;
            }
        } else if (held.bytes == 0 && !reserve_scratch(held, per_sample * chunk, realloc)) {
            plan.error = "no device memory for the parked samples";
            return BT_ERR_DEVICE;
        }
    }
    plan.parked_bytes = px_launch * T_all * sample_bytes;
    if (guided) {
        // the guides' planes behind the colour values of the launch, each indexed like them (bt_types.h guide_scratch)
        uint64_t plane = values * 3;
        for (int g = 0; g < 3; ++g)
            if (guides >> g & 1u) {
                plan.guide_values[g] = plane;
                plane += values * (g == 2 ? 1 : 3);
            }
        if (plane * sizeof(float) > held.bytes) {
            plan.error = "the guides' parked values do not fit the scratch";
            return BT_ERR_DEVICE;
        }
    }

    if (lds_bytes > 158 * 1024) {
        plan.error = "scene tables (" + std::to_string(flat.lds_bytes()) + " bytes) exceed the 160 KB of LDS of a gfx950 CU";
        return BT_ERR_INVALID_ARG;
    }
    // longest wait in iterations (0 = no voting); measured best: 3 on scene.json, 4 on the volume scenes
    // (profiles/r01f/ab_phase_vote.log, profiles/r01g/ab_vote_both.log)
    P.phase_vote = tune.phase_vote >= 0 ? tune.phase_vote : (P.any_volumes ? 4 : 3);
    plan.chunk = chunk;
    plan.launches = ((uint32_t)P.samples + chunk - 1) / chunk;
    plan.lds_bytes = lds_bytes;
    plan.pixels = pixels_owned(P.width, P.height, P.rank, P.world);
    return 0;
}

// What bt_stats says about a planned render (the counters and the time come from the device).
inline void plan_stats(const BtLaunch &P, const Plan &plan, const Scratch &held, bt_stats &st) {
    st.pixels = plan.pixels;
    st.samples = plan.pixels * (uint64_t)P.samples * (uint64_t)(P.subsample_n * P.subsample_n);
    st.segments = 0;
    st.kernel_ms = 0.0f;
    st.slices = (uint32_t)P.slices;
    st.launches = plan.launches;
    st.packed = P.wg_blocks > 1 ? (P.pool_records ? 2u : 1u) : 0u;
    st.workgroups = P.wg_blocks > 1 ? P.n_workgroups : plan.grid * (uint32_t)P.slices;
    st.scratch_bytes = held.bytes;
    st.parked_bytes = plan.parked_bytes;
}

} // namespace btplan
