// bt_internal.hpp -- everything that crosses translation units inside libbendy_hip.so and is not in include/bendy_hip.h.
// Included by the file that defines each of these and by the files that call it: a declaration that does not match its
// definition does not compile.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/bendy_hip.h"
#include "bt_view.hpp"

struct BtLaunch;
struct BtSphereRow;

// One launch of the temporal kernel (bt_temporal.hip), passed by value.  The planes are width * height float4 each.
struct BtTemporalLaunch {
    btview::View cur, prev;                  // prev: read by the reprojecting build only
    const float4 *color, *normal, *depth;    // this frame's running sums; normal may be null
    float nc, nn, nd;                        // their sample counts
    const float4 *hist_in, *guide_in;        // the previous frame's history (rgb = mean, a = length) and guides (n.xyz, z)
    float4 *hist_out, *guide_out, *out;
    float alpha_min, max_history, depth_tolerance, normal_min;
};

// The display stage (bt_display.hip).  A handle's device memory is uint32 words: the live counters (256 luminance bins, then
// `under`, then `over`), the last call's counters for bt_debug_display_histogram, then one BtDisplayState.
#define BT_DISPLAY_BINS 256
#define BT_DISPLAY_COUNTERS 258
#define BT_DISPLAY_STRIDE 260                // counters padded to 16 B
struct BtDisplayState {
    float e;                                 // the adapted exposure, meaningful while `valid`
    uint32_t valid;
    float shown_ev, shown_mult;              // what the last call's frame was shown with (bt_display_exposure)
};
struct BtDisplayExpose {
    double log2_key;                         // log2(key), formed once on the host
    float p_low, p_high, ev, ev_min, ev_max, adapt;
};

// The ray query API (bt_query.hip).  One BtQueryRef per row of the primitive table, uploaded next to it: what the
// row's hit reports besides geometry (UINT64_MAX: no volume).
struct BtQueryRef {
    uint64_t object_ref, material_ref, volume_ref;
};
struct BtPrim;
struct BtQueryLaunch {
    const BtPrim *prims;
    const BtQueryRef *refs;
    const bt_ray *rays;
    bt_hit *hits;
    int32_t n_prims;
    uint32_t n;                              // rays, 0 < n < 2^30
};
struct BtViewRaysLaunch {
    btview::View view;
    uint32_t x0, y0, w, h;                   // the rectangle, inside the view's frame; w * h < 2^30
    bt_ray *rays;
};

extern "C" {
// bt_kernels.hip
hipError_t bt_launch_render(const BtLaunch *P, int output, unsigned grid, size_t lds_bytes, hipStream_t stream);
hipError_t bt_launch_unshard(const float *gathered, float *frame, uint32_t width, uint32_t height, uint32_t tiles_x,
                             uint32_t tiles_y, uint32_t world, uint32_t tiles_per_rank, hipStream_t stream);
void bt_primary_masks_host(const BtLaunch *P, const BtSphereRow *rows, uint32_t n_blocks, uint64_t *out);
int bt_launch_reads_masks(const BtLaunch *P, int output);
int bt_mask_cache_enabled(void);
hipError_t bt_launch_block_masks(const BtLaunch *P, uint32_t n_blocks, uint64_t *masks, hipStream_t stream);
// out: BT_ORDER_HEADER + n_blocks words (bt_cull.hpp block_order)
hipError_t bt_launch_block_order(const uint64_t *masks, uint32_t n_blocks, uint32_t *out, hipStream_t stream);
hipError_t bt_launch_philox_test(const uint32_t *pairs, uint32_t n, uint32_t *out, hipStream_t stream);
hipError_t bt_launch_preview(const float *rgba, uint8_t *out, uint32_t n, uint32_t samples, int color_space, hipStream_t stream);
// bt_adapt.hip
hipError_t bt_launch_adapt_update(const float *rgba, const float *moment, uint32_t *count, uint32_t *active, float *error,
                                  uint32_t *n_active, uint32_t width, uint32_t height, uint32_t T, const bt_adaptive_params *p,
                                  hipStream_t stream);
hipError_t bt_launch_adapt_resolve(const float *rgba, const uint32_t *count, float *out, uint32_t width, uint32_t height,
                                   hipStream_t stream);
// bt_denoise.hip
hipError_t bt_launch_denoise(const float *color, float nc, const float *albedo, float na, const float *normal, float nn,
                             const float *depth, float nd, float *out, float *e0, float *e1, float *guide, uint32_t width,
                             uint32_t height, uint32_t levels, float sigma_color, float sigma_normal, float sigma_depth,
                             float eps_albedo, hipStream_t stream);
// bt_temporal.hip: mode 0 = no history, 1 = the previous view again, 2 = reproject
hipError_t bt_launch_temporal(const BtTemporalLaunch *P, int mode, hipStream_t stream);
// bt_display.hip: `op` is a bt_tonemap; `manual` != 0: the frame is shown with `ev`, the state's (e, valid) is not read
hipError_t bt_launch_display_meter(const float *rgba, uint64_t n, uint32_t samples, uint32_t *live, hipStream_t stream);
hipError_t bt_launch_display_expose(uint32_t *live, uint32_t *last, BtDisplayState *state, const BtDisplayExpose *p,
                                    hipStream_t stream);
hipError_t bt_launch_display_show(const float *rgba, uint8_t *out, uint64_t n, uint32_t samples, int color_space, int op,
                                  float iw2, int manual, float ev, BtDisplayState *state, hipStream_t stream);
// bt_query.hip
hipError_t bt_launch_query(const BtQueryLaunch *Q, hipStream_t stream);
hipError_t bt_launch_view_rays(const BtViewRaysLaunch *P, hipStream_t stream);
// bt_api.cpp
// The ray query's way to the scene: flattens and uploads the tables if they are stale (BT_ERR_DEVICE without a device) and hands
// out the device pointers of the primitive table and of its BtQueryRef table.  Touches no render state of the handle.
int bt_scene_query_tables_internal(bt_scene *scene, const BtPrim **prims, const BtQueryRef **refs, int32_t *n_prims);
int bt_set_error_internal(int code, const char *msg);      // sets bt_last_error / bt_last_error_code; returns `code`
int bt_scene_lens_on_internal(const bt_scene *scene);
// The render half of bt_render_adaptive_device (bt_adapt_api.cpp, which has validated everything).
int bt_render_adaptive_pass_internal(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                                     float *rgba_device, uint32_t width, uint32_t height, uint64_t seed, void *stream,
                                     const uint32_t *tile_active, float *moment);
}

static inline int fail(int code, const std::string &msg) { return bt_set_error_internal(code, msg.c_str()); }
static inline int hip_fail(const char *what, hipError_t e) { return fail(BT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }
#define BT_HIP(expr)                                        \
    do {                                                    \
        hipError_t _e = (expr);                             \
        if (_e != hipSuccess) return hip_fail(#expr, _e);   \
    } while (0)
