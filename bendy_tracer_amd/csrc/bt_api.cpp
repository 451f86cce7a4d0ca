// bt_api.cpp -- the C ABI of libbendy_hip.so (include/bendy_hip.h): scene handles, parameter
// preparation for Tracer::render (reference tracer/mod.rs:179-320) and kernel launches.
// There is no CPU fallback: without a HIP device every render entry point returns BT_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/bendy_hip.h"
#include "bt_internal.hpp"
#include "bt_scene.hpp"
#include "bt_types.h"
#include "bt_cull.hpp"
#include "bt_plan.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

thread_local std::string g_error;
thread_local int g_error_code = 0;
constexpr uint32_t kCounterSlots = 64;                // work counters: one memset per 64 renders instead of one per render

template <class T> struct DeviceArray {
    T *ptr = nullptr;
    size_t count = 0;
    ~DeviceArray() { release(); }
    size_t bytes() const { return sizeof(T) * count; }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        count = 0;
    }
    hipError_t allocate(size_t n) {                    // n elements, contents undefined
        release();
        hipError_t e = hipMalloc((void **)&ptr, sizeof(T) * n);
        if (e == hipSuccess) count = n;
        return e;
    }
    hipError_t upload(const std::vector<T> &src) {
        hipError_t e = allocate(src.size() ? src.size() : 1);
        count = src.size();
        if (e == hipSuccess && count) e = hipMemcpy(ptr, src.data(), sizeof(T) * count, hipMemcpyHostToDevice);
        return e;
    }
};

} // namespace

struct bt_scene {
    bt::Scene scene;
    std::string source;            // the JSON document the scene was parsed from (for bt_scene_save)
    bt::FlatScene flat;
    bool flat_valid = false;
    bool device_valid = false;
    int device = -1;
    DeviceArray<BtPrim> d_prims;
    DeviceArray<BtMaterial> d_materials;
    DeviceArray<BtVolume> d_volumes;
    DeviceArray<BtLight> d_lights;
    DeviceArray<BtLightFace> d_light_faces;
    DeviceArray<BtSpherePair> d_sphere_pairs;
    DeviceArray<BtSphereRow> d_sphere_rows;
    DeviceArray<BtRectAAN> d_aan_rows;
    DeviceArray<BtRectLA> d_la_rows;
    DeviceArray<int32_t> d_other_rows;
    DeviceArray<float> d_density;
    DeviceArray<BtQueryRef> d_query_refs;  // ray query extension: one row per row of d_prims (bt_internal.hpp)
    DeviceArray<int32_t> d_lens_prims;     // lens extension: rows of d_prims near the sphere of influence
    bt_lens lens_prims_for{};              // the lens d_lens_prims was built for
    bool lens_prims_valid = false;
    unsigned long long *d_counters = nullptr;   // kCounterSlots x 16 words: render number n counts into slot n mod kCounterSlots
    uint32_t render_seq = 0;       // renders issued on this handle (selects the counter slot)
    uint32_t last_slot = 0;
    DeviceArray<float> d_scratch;  // parked sample values of sliced renders
    uint32_t scratch_small_streak = 0;   // consecutive renders that needed less than a quarter of the scratch held
    btplan::Scratch plan_scratch;  // the scratch bt_debug_plan_launch plans with: a number, no device memory
    // per-block sphere masks of the last launch that read them (bt_cull.hpp block_mask): grow-only, reused as long as the key
    // -- everything the masks depend on -- stays what it was (a progressive sequence, the launches of one deep render)
    DeviceArray<uint64_t> d_block_masks;
    DeviceArray<uint32_t> d_block_order;   // {n_live, n_empty, order[]} made from those masks (bt_cull.hpp block_order): same key
    btcull::MaskKey masks_for{};   // valid = 0: none
    uint64_t rows_generation = 0;  // bumped wherever d_sphere_rows is uploaded
    DeviceArray<float> d_host_frame;   // device copy of the caller's host buffer (bt_render), kept between calls
    int n_cu = 0;                  // hipDeviceProp_t::multiProcessorCount of `device`
    bt_tuning tuning{};            // bt_scene_set_tuning; zero / negative fields = automatic
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bt_stats last{};
    bool lens_on = false;          // lens extension (not in the reference), bt_scene_set_lens
    bt_lens lens{};
    bool stats_pending = false;

    bt_scene() { bt_tuning_default(&tuning); }
    // everything that lives on `device` besides the scene tables (which upload() replaces)
    void release_device_state() {
        if (d_counters) (void)hipFree(d_counters);
        if (ev_start) (void)hipEventDestroy(ev_start);
        if (ev_stop) (void)hipEventDestroy(ev_stop);
        d_counters = nullptr;
        ev_start = ev_stop = nullptr;
        stats_pending = false;
        release_buffers();
    }
    // what the handle keeps between calls and bt_scene_trim gives back: the scratch, the cached host frame, the block masks
    void release_buffers() {
        d_scratch.release();
        d_host_frame.release();
        d_block_masks.release();
        d_block_order.release();
        masks_for = btcull::MaskKey{};
        scratch_small_streak = 0;
    }
    ~bt_scene() { release_device_state(); }
};

namespace {

int ensure_flat(bt_scene *s) {
    if (s->flat_valid) return 0;
    try {
        s->flat = bt::flatten_scene(s->scene);
    } catch (const bt::Error &e) {
        return fail(e.code, e.message);
    }
    s->flat_valid = true;
    s->device_valid = false;
    s->rows_generation += 1;                       // new rows (part of the block masks' key); the upload bumps it again
    return 0;
}

// BtSphereRow table of a sphere-only scene (bt_types.h), empty when any row is not a sphere
std::vector<BtSphereRow> sphere_rows_of(const std::vector<BtPrim> &pr) {
    std::vector<BtSphereRow> rows;
    bool spheres_only = true;
    for (const BtPrim &R : pr) spheres_only = spheres_only && (R.kind & BT_PRIM_SHAPE_MASK) == BT_PRIM_SPHERE;
    if (spheres_only)
        for (const BtPrim &R : pr) rows.push_back(BtSphereRow{R.c.x, R.c.y, R.c.z, R.radius * R.radius});
    if (rows.size() & 1) rows.push_back(rows.back());           // (never visited: keeps an x8 load of the last pair inside the table)
    return rows;
}

// BtQueryRef table of the flattened scene (ray query extension): the refs behind each row's object, material and volume index.
// flatten_scene numbers materials and volumes in the order of the scene's data, each kind on its own.
std::vector<BtQueryRef> query_refs_of(const bt::Scene &sc, const std::vector<BtPrim> &pr) {
    std::vector<uint64_t> mat_ref, vol_ref;
    for (const bt::Data &d : sc.data) (d.kind == bt::DATA_VOLUME ? vol_ref : mat_ref).push_back(d.data_ref);
    std::vector<BtQueryRef> refs;
    for (const BtPrim &R : pr)
        refs.push_back(BtQueryRef{sc.objects[(size_t)R.object].object_ref, mat_ref[(size_t)R.material],
                                  R.volume >= 0 ? vol_ref[(size_t)R.volume] : ~0ull});
    return refs;
}

int ensure_device(bt_scene *s) {
    int rc = ensure_flat(s);
    if (rc) return rc;
    int dev = -1;
    BT_HIP(hipGetDevice(&dev));
    if (s->device_valid && s->device == dev) return 0;
    if (s->device >= 0 && s->device != dev) {
        // the handle moves to another GPU: counters, scratch, the cached host frame and the events belong to the old
        // one (a kernel on `dev` must not write into them) -- free them there and start afresh here
        (void)hipSetDevice(s->device);
        s->release_device_state();
        BT_HIP(hipSetDevice(dev));
    }
    {
        hipDeviceProp_t prop;
        BT_HIP(hipGetDeviceProperties(&prop, dev));
        s->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    BT_HIP(s->d_prims.upload(s->flat.prims));
    BT_HIP(s->d_materials.upload(s->flat.materials));
    BT_HIP(s->d_volumes.upload(s->flat.volumes));
    BT_HIP(s->d_lights.upload(s->flat.lights));
    BT_HIP(s->d_light_faces.upload(s->flat.light_faces));
    {
        std::vector<BtSpherePair> pairs;
        const std::vector<BtPrim> &pr = s->flat.prims;
        bool spheres_only = true;
        for (const BtPrim &R : pr) spheres_only = spheres_only && (R.kind & BT_PRIM_SHAPE_MASK) == BT_PRIM_SPHERE;
        if (spheres_only)
            for (size_t i = 0; i < pr.size(); i += 2) {
                const BtPrim &A = pr[i], &B = pr[i + 1 < pr.size() ? i + 1 : i];
                BtSpherePair q{};
                q.cx[0] = A.c.x; q.cy[0] = A.c.y; q.cz[0] = A.c.z; q.radius[0] = A.radius; q.object[0] = A.object;
                q.cx[1] = B.c.x; q.cy[1] = B.c.y; q.cz[1] = B.c.z; q.radius[1] = B.radius; q.object[1] = B.object;
                pairs.push_back(q);
            }
        BT_HIP(s->d_sphere_pairs.upload(pairs));
        BT_HIP(s->d_sphere_rows.upload(sphere_rows_of(pr)));
        s->rows_generation += 1;                   // (part of the block masks' key)
    }
    BT_HIP(s->d_density.upload(s->flat.density));
    BT_HIP(s->d_query_refs.upload(query_refs_of(s->scene, s->flat.prims)));
    BT_HIP(s->d_aan_rows.upload(s->flat.aan_rows));
    BT_HIP(s->d_la_rows.upload(s->flat.la_rows));
    BT_HIP(s->d_other_rows.upload(s->flat.other_rows));
    if (!s->d_counters) {
        BT_HIP(hipMalloc((void **)&s->d_counters, kCounterSlots * 16 * sizeof(unsigned long long)));
        s->render_seq = 0;
    }
    if (!s->ev_start) BT_HIP(hipEventCreate(&s->ev_start));
    if (!s->ev_stop) BT_HIP(hipEventCreate(&s->ev_stop));
    s->device = dev;
    s->device_valid = true;
    s->lens_prims_valid = false;
    return 0;
}

// Lens extension: rows of the primitive table whose surface can come within `reach` of the lens centre.
// Conservative by construction (double arithmetic, bounding spheres for rects, 0.1 % slack): a row that is left
// out cannot be touched by any point within `reach` of the centre.
std::vector<int32_t> lens_candidates(const std::vector<BtPrim> &prims, const bt_lens &lens, double reach) {
    std::vector<int32_t> rows;
    const double cx = lens.centre[0], cy = lens.centre[1], cz = lens.centre[2];
    reach *= 1.001;
    for (size_t i = 0; i < prims.size(); ++i) {
        const BtPrim &R = prims[i];
        bool near_ = true;
        if ((R.kind & BT_PRIM_SHAPE_MASK) == BT_PRIM_SPHERE) {
            const double d = std::sqrt((R.c.x - cx) * (R.c.x - cx) + (R.c.y - cy) * (R.c.y - cy) + (R.c.z - cz) * (R.c.z - cz));
            near_ = std::fabs(d - (double)R.radius) <= reach + 1e-3 * (double)R.radius;    // the SURFACE is what is hit
        } else {
            // forward matrix = inverse of (icx, icy, icz); corners = t + M * (+-hw * ax +- hh * ay)
            const double a[3][3] = {{R.icx.x, R.icy.x, R.icz.x}, {R.icx.y, R.icy.y, R.icz.y}, {R.icx.z, R.icy.z, R.icz.z}};
            const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                               a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
            if (std::isfinite(det) && std::fabs(det) > 1e-30) {
                double m[3][3];
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) {
                        const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
                        m[r][c] = (a[r1][c1] * a[r2][c2] - a[r1][c2] * a[r2][c1]) / det;
                    }
                const double hw = std::sqrt((double)R.w_sqr), hh = std::sqrt((double)R.h_sqr);
                // local axes: Rect.x / Rect.y, which BT_PRIM_RECT_LA / _AAN rows replace by other constants (bt_types.h)
                double lx[3] = {R.ax.x, R.ax.y, R.ax.z}, ly[3] = {R.ay.x, R.ay.y, R.ay.z};
                if ((R.kind & BT_PRIM_SHAPE_MASK) == BT_PRIM_RECT_LA || (R.kind & BT_PRIM_SHAPE_MASK) == BT_PRIM_RECT_AAN)
                    for (int i = 0; i < 3; ++i) {
                        lx[i] = i == R.aa_u ? 1.0 : 0.0;
                        ly[i] = i == R.aa_v ? 1.0 : 0.0;
                    }
                double bound = 0.0;
                for (int sx = -1; sx <= 1; sx += 2)
                    for (int sy = -1; sy <= 1; sy += 2) {
                        const double l[3] = {sx * hw * lx[0] + sy * hh * ly[0], sx * hw * lx[1] + sy * hh * ly[1],
                                             sx * hw * lx[2] + sy * hh * ly[2]};
                        double wv[3];
                        for (int r = 0; r < 3; ++r) wv[r] = m[r][0] * l[0] + m[r][1] * l[1] + m[r][2] * l[2];
                        bound = std::max(bound, std::sqrt(wv[0] * wv[0] + wv[1] * wv[1] + wv[2] * wv[2]));
                    }
                const double d = std::sqrt((R.t.x - cx) * (R.t.x - cx) + (R.t.y - cy) * (R.t.y - cy) + (R.t.z - cz) * (R.t.z - cz));
                near_ = d - bound * 1.001 <= reach;
            }
        }
        if (near_) rows.push_back((int32_t)i);
    }
    return rows;
}

// ChunkConfig::with_configs (mod.rs:217-229) + camera setup (mod.rs:244-267)
int fill_launch(bt_scene *s, uint64_t camera_ref, const bt_config *cfg, const bt_render_config *rc, uint32_t width,
                uint32_t height, uint64_t seed, BtLaunch &P, int &output) {
    if (!s || !cfg || !rc) return fail(BT_ERR_INVALID_ARG, "null argument");
    if (width == 0 || height == 0) return fail(BT_ERR_INVALID_ARG, "zero-sized buffer");
    int ci = s->scene.object_index(camera_ref);
    if (ci < 0) return fail(BT_ERR_INVALID_REF, "invalid object ref " + std::to_string(camera_ref));
    const bt::Object &cam = s->scene.objects[ci];
    if (cam.kind != bt::OBJ_CAMERA) return fail(BT_ERR_NOT_CAMERA, "expected a camera object");

    std::memset(&P, 0, sizeof P);
    const bt::FlatScene &f = s->flat;
    P.prims = s->d_prims.ptr;
    P.materials = s->d_materials.ptr;
    P.volumes = s->d_volumes.ptr;
    P.lights = s->d_lights.ptr;
    P.light_faces = s->d_light_faces.ptr;
    P.sphere_pairs = s->d_sphere_pairs.count ? s->d_sphere_pairs.ptr : nullptr;
    P.sphere_rows = s->d_sphere_rows.count ? s->d_sphere_rows.ptr : nullptr;
    P.density = s->d_density.ptr;
    P.n_prims = (int32_t)f.prims.size();
    P.n_materials = (int32_t)f.materials.size();
    P.n_volumes = (int32_t)f.volumes.size();
    P.n_lights = (int32_t)f.lights.size();
    P.n_light_faces = (int32_t)f.light_faces.size();
    P.n_density = (int32_t)f.density.size();
    P.any_rects = 0;
    for (const BtPrim &R : f.prims)
        if ((R.kind & BT_PRIM_SHAPE_MASK) != BT_PRIM_SPHERE) P.any_rects = 1;
    P.any_volumes = btplan::any_prim_carries_volume(f.prims) ? 1 : 0;
    P.aan_rows = s->d_aan_rows.ptr;
    P.la_rows = s->d_la_rows.ptr;
    P.n_la = (int32_t)f.la_rows.size();
    P.other_rows = s->d_other_rows.ptr;
    P.n_aan[0] = f.n_aan[0]; P.n_aan[1] = f.n_aan[1]; P.n_aan[2] = f.n_aan[2];
    P.n_other = (int32_t)f.other_rows.size();
    P.root_color = f.root_color;
    P.root_albedo = f.root_albedo;
    P.root_has_albedo = f.root_has_albedo;

    P.cam_cx = cam.world.cx; P.cam_cy = cam.world.cy; P.cam_cz = cam.world.cz; P.cam_t = cam.world.t;
    P.yfov = 2.0f * atan2f(cam.sensor_size, 2.0f * cam.focal_length);  // mod.rs:248
    P.xfov = P.yfov * cam.aspect_ratio;                                // mod.rs:249
    P.pixel_width = 2.0f * (1.0f / (float)width);                      // buffer.rs:68-71
    P.pixel_height = 2.0f * (1.0f / (float)height);                    // buffer.rs:73-76
    const uint32_t n = rc->subsample_n >= 2 ? rc->subsample_n : 1;     // mod.rs:47-67, main.rs:234-237
    const float subpixel_scale = rc->subsample_n >= 2 ? 1.0f / (float)rc->subsample_n : 1.0f;
    const float umin = -0.5f * P.pixel_width * subpixel_scale, umax = 0.5f * P.pixel_width * subpixel_scale;
    const float vmin = -0.5f * P.pixel_height * subpixel_scale, vmax = 0.5f * P.pixel_height * subpixel_scale;
    P.jitter_u_lo = umin;
    P.jitter_u_scale = bt::uniform_scale(umin, umax, false);           // mod.rs:255-259
    P.jitter_v_lo = vmin;
    P.jitter_v_scale = bt::uniform_scale(vmin, vmax, false);           // mod.rs:261-265
    P.has_focus = cam.has_focus ? 1 : 0;
    P.focus = cam.focus;
    P.aperture = 0.5f * cam.focal_length / cam.fstop;                  // mod.rs:289
    BtV3 neg_z; neg_z.x = 0.0f; neg_z.y = 0.0f; neg_z.z = -1.0f;      // UnitDisk::new(Vec3::NEG_Z), mod.rs:267
    bt::orthonormal_pair(neg_z, P.disk_x, P.disk_y);
    P.tau_scale = bt::uniform_scale(0.0f, 6.28318530717958647692f, true);
    P.one_scale = bt::uniform_scale(0.0f, 1.0f, true);

    output = rc->has_output ? rc->output : cfg->output;                // mod.rs:220
    if (output < 0 || output > 3) return fail(BT_ERR_INVALID_ARG, "invalid output mode");
    P.max_bounces = (int32_t)(rc->has_max_bounces ? rc->max_bounces : cfg->max_bounces);                 // :223
    P.max_volume_bounces = (int32_t)(rc->has_max_bounces ? rc->max_bounces : cfg->max_volume_bounces);   // :224 (Q1)
    P.clip_min = cfg->clip_min;
    P.clip_max = cfg->clip_max;
    P.volume_step = rc->has_volume_step ? rc->volume_step : cfg->volume_step;                            // :227
    // The build for rect scenes without volumes walks the sorted tables with a division whose range handling is hoisted
    // out (bt_device.hpp div_refined): valid for 2^-30 <= clip_min, clip_max <= 2^60 and row ranks that fit 15 bits.  Any
    // other rect scene runs the generic loop, which lives in the rects + volumes build.
    if (P.any_rects && !P.any_volumes &&
        !(P.clip_min >= 0x1p-30f && P.clip_max <= 0x1p60f && f.prims.size() < 0x7fffu))
        P.any_volumes = 1;
    if (rc->samples > 0x7fffffffu / (n * n)) return fail(BT_ERR_INVALID_ARG, "samples * n^2 overflows");
    P.samples = (int32_t)rc->samples;
    P.subsample_n = (int32_t)n;
    P.sample_base = rc->sample_base;
    P.seed_lo = (uint32_t)seed;
    P.seed_hi = (uint32_t)(seed >> 32);
    P.width = width;
    P.height = height;
    P.tiles_x = btplan::tiles_across(width);
    P.tiles_x_magic = P.tiles_x == 1 ? 0xffffffffu : (uint32_t)(0x100000000ull / P.tiles_x);   // kernels: tile / tiles_x by umulhi + one fix-up
    P.tiles_y = btplan::tiles_across(height);
    P.rank = 0;
    P.world = 1;
    P.sharded = 0;
    P.counters = s->d_counters;                 // (render_common points it at this render's slot)
    P.lens_on = s->lens_on ? 1 : 0;
    P.lens_c.x = s->lens.centre[0]; P.lens_c.y = s->lens.centre[1]; P.lens_c.z = s->lens.centre[2];
    P.lens_rs = s->lens.rs;
    P.lens_step = s->lens.step;
    P.lens_radius = s->lens.radius;
    P.lens_max_steps = (int32_t)s->lens.max_steps;
    P.lens_prims = nullptr;                     // (render_common uploads the candidates: upload_lens_prims)
    P.n_lens_prims = 0;
    // |v| <= sqrt(1 + rs h^2 / r^3) <= 2.8 along any geodesic that started with |v| = 1 (h^2 <= 6.75 rs^2 for the
    // captured ones, r >= rs), so a chord is at most ~2.8 steps long; longer ones (never seen) fall back to the
    // full table in the kernel
    P.lens_margin = s->lens_on ? 3.0f * s->lens.step : 0.0f;
    return 0;
}

// The lens extension's candidate rows for the lens `P` was filled for (lens_candidates), uploaded when the lens changed.
int upload_lens_prims(bt_scene *s, BtLaunch &P) {
    if (!s->lens_on) return 0;
    if (!s->lens_prims_valid || std::memcmp(&s->lens_prims_for, &s->lens, sizeof(bt_lens)) != 0) {
        BT_HIP(s->d_lens_prims.upload(lens_candidates(s->flat.prims, s->lens, (double)s->lens.radius + (double)P.lens_margin)));
        s->lens_prims_for = s->lens;
        s->lens_prims_valid = true;
    }
    P.lens_prims = s->d_lens_prims.ptr;
    P.n_lens_prims = (int32_t)s->d_lens_prims.count;
    return 0;
}

// One mask per block and the block order made from the masks, the same for every launch of this render (blocks and slices do
// not change with the sample range) and for every later render with the same key; computed on this stream, inside the timed
// region, the order kernel behind the mask kernel.
int ensure_block_masks(bt_scene *s, BtLaunch &P, uint32_t n_blocks, hipStream_t stream) {
    btcull::MaskKey key;
    btcull::mask_key(key, P, n_blocks, s->rows_generation, (const void *)stream);
    if (!bt_mask_cache_enabled() || std::memcmp(&key, &s->masks_for, sizeof key) != 0) {
        if (s->d_block_masks.count < n_blocks || s->d_block_order.count < (size_t)n_blocks + BT_ORDER_HEADER) {
            if (s->d_block_masks.ptr) BT_HIP(hipDeviceSynchronize());    // earlier launches, on whichever stream, may still read the old buffers
            s->masks_for = btcull::MaskKey{};
            BT_HIP(s->d_block_masks.allocate(n_blocks));
            BT_HIP(s->d_block_order.allocate((size_t)n_blocks + BT_ORDER_HEADER));
        }
        s->masks_for = btcull::MaskKey{};          // (stays invalid if a launch fails)
        BT_HIP(bt_launch_block_masks(&P, n_blocks, s->d_block_masks.ptr, stream));
        BT_HIP(bt_launch_block_order(s->d_block_masks.ptr, n_blocks, s->d_block_order.ptr, stream));
        s->masks_for = key;
    }
    P.block_masks = s->d_block_masks.ptr;
    P.block_order = s->d_block_order.ptr;
    return 0;
}

// btplan::reserve_scratch's way to device memory: frees the scratch held, allocates `need` bytes; the bytes held afterwards.
uint64_t realloc_scratch(bt_scene *s, hipStream_t stream, uint64_t need) {
    if (s->d_scratch.ptr && hipStreamSynchronize(stream) != hipSuccess) return s->d_scratch.bytes();   // an earlier launch on this stream may still read it
    s->d_scratch.release();
    if (need && s->d_scratch.allocate(need / sizeof(float)) != hipSuccess) (void)hipGetLastError();
    return s->d_scratch.bytes();
}

// The kind of pass.  GUIDED (bt_render_guided_device, an extension): the albedo / normal / depth frames, any of them null; the
// caller has checked that the effective output is BT_OUTPUT_FULL and that no lens is set.  ADAPTIVE (bt_render_adaptive_device,
// an extension; bt_adapt_api.cpp): the per-tile activity flags and the moment plane of one adaptive pass; the caller has
// checked the same two things.
struct RenderPass {
    int kind = btplan::PLAIN;
    float *guides[3] = {nullptr, nullptr, nullptr};
    const uint32_t *tile_active = nullptr;
    float *moment = nullptr;
    uint32_t guide_mask() const { return (guides[0] ? 1u : 0u) | (guides[1] ? 2u : 0u) | (guides[2] ? 4u : 0u); }
};

// The device half of a render: what to launch is btplan::plan_launch's decision (bt_plan.hpp).
int render_common(bt_scene *s, uint64_t camera_ref, const bt_config *cfg, const bt_render_config *rc, float *out_device,
                  uint32_t width, uint32_t height, uint32_t rank, uint32_t world, bool sharded, uint64_t seed,
                  hipStream_t stream, const RenderPass &pass = RenderPass{}) {
    if (!s || !cfg || !rc || !out_device) return fail(BT_ERR_INVALID_ARG, "null argument");
    if (rc->samples == 0) return BT_DONE;                              // mod.rs:186-188
    if (world == 0 || rank >= world) return fail(BT_ERR_INVALID_ARG, "rank/world out of range");
    int rcode = ensure_device(s);
    if (rcode) return rcode;
    BtLaunch P;
    int output = 0;
    rcode = fill_launch(s, camera_ref, cfg, rc, width, height, seed, P, output);
    if (rcode) return rcode;
    rcode = upload_lens_prims(s, P);
    if (rcode) return rcode;
    btplan::shard_launch(P, rank, world, sharded);
    P.out = out_device;

    btplan::Plan plan;
    btplan::Scratch held{s->d_scratch.bytes(), s->scratch_small_streak};
    rcode = btplan::plan_launch(P, output, s->flat, s->tuning, (uint32_t)s->n_cu, pass.kind, pass.guide_mask(), held,
                                [&](uint64_t need) { return realloc_scratch(s, stream, need); }, plan);
    s->scratch_small_streak = held.small_streak;
    if (rcode) return fail(rcode, plan.error);
    P.scratch = s->d_scratch.ptr;
    for (int g = 0; g < 3; ++g) {
        P.guide_out[g] = plan.output == 4 ? pass.guides[g] : nullptr;
        P.guide_scratch[g] = plan.guide_values[g] ? P.scratch + plan.guide_values[g] : nullptr;
    }
    P.tile_active = pass.tile_active;
    P.moment = pass.moment;

    // work counters: a ring of slots, zeroed all at once when the ring wraps -- the interactive loop (main.rs:245-254, one
    // render per displayed frame) then pays one memset per 64 frames instead of one per frame in front of a 0.1 ms kernel
    s->last_slot = s->render_seq % kCounterSlots;
    if (s->last_slot == 0) BT_HIP(hipMemsetAsync(s->d_counters, 0, kCounterSlots * 16 * sizeof(unsigned long long), stream));
    s->render_seq += 1;
    P.counters = s->d_counters + (size_t)s->last_slot * 16;
    BT_HIP(hipEventRecord(s->ev_start, stream));
    P.block_masks = nullptr;
    P.block_order = nullptr;
    if (bt_launch_reads_masks(&P, plan.output)) {
        rcode = ensure_block_masks(s, P, plan.grid * (uint32_t)P.slices, stream);
        if (rcode) return rcode;
    }
    {
        const uint32_t all = (uint32_t)P.samples, base = P.sample_base;
        for (uint32_t done = 0; done < all; done += plan.chunk) {
            P.samples = (int32_t)std::min(plan.chunk, all - done);
            P.sample_base = base + done;
            BT_HIP(bt_launch_render(&P, plan.output, plan.grid, plan.lds_bytes, stream));
        }
        P.samples = (int32_t)all;
        P.sample_base = base;
    }
    BT_HIP(hipEventRecord(s->ev_stop, stream));

    btplan::plan_stats(P, plan, held, s->last);
    s->stats_pending = true;
    return BT_IN_PROGRESS;                                             // mod.rs:201
}

} // namespace

extern "C" {

void bt_config_default(bt_config *c) {
    if (!c) return;
    c->max_bounces = 8;
    c->max_volume_bounces = 32;
    c->clip_min = 0.01f;
    c->clip_max = 1000.0f;
    c->volume_step = 0.1f;
    c->chunks_x = 4;
    c->chunks_y = 2;
    c->output = BT_OUTPUT_FULL;
}

void bt_render_config_default(bt_render_config *r) {
    if (!r) return;
    std::memset(r, 0, sizeof *r);
    r->samples = 64;
}

const char *bt_last_error(void) { return g_error.c_str(); }
int bt_set_error_internal(int code, const char *msg) {
    g_error = msg ? msg : "";
    g_error_code = code;
    return code;
}
int bt_last_error_code(void) { return g_error_code; }

void bt_tuning_default(bt_tuning *t) {
    if (!t) return;
    std::memset(t, 0, sizeof *t);
    t->phase_vote = -1;
    t->packed = -1;
}

int bt_scene_set_tuning(bt_scene *scene, const bt_tuning *t) {
    if (!scene) return fail(BT_ERR_INVALID_ARG, "null scene");
    if (!t) {
        bt_tuning_default(&scene->tuning);
        return 0;
    }
    const uint32_t S = t->slices;
    if (!(S == 0 || S == 1 || S == 2 || S == 4 || S == 8 || S == 16 || S == 32))
        return fail(BT_ERR_INVALID_ARG, "bt_tuning.slices must be 0 (auto), 1, 2, 4, 8, 16 or 32");
    if (t->phase_vote < -1 || t->phase_vote > 64)
        return fail(BT_ERR_INVALID_ARG, "bt_tuning.phase_vote must be -1 .. 64");
    if (t->packed < -1 || t->packed > 2) return fail(BT_ERR_INVALID_ARG, "bt_tuning.packed must be -1, 0, 1 or 2");
    scene->tuning = *t;
    return 0;
}

int bt_scene_get_tuning(const bt_scene *scene, bt_tuning *out) {
    if (!scene || !out) return fail(BT_ERR_INVALID_ARG, "null argument");
    *out = scene->tuning;
    return 0;
}

const char *bt_version(void) { return "bendy-hip 0.1 (gfx950)"; }

bt_scene *bt_scene_from_json(const char *json, size_t len) {
    if (!json) {
        fail(BT_ERR_INVALID_ARG, "null json");
        return nullptr;
    }
    try {
        std::unique_ptr<bt_scene> s(new bt_scene());
        s->scene = bt::parse_scene(json, len);
        s->source.assign(json, len);
        return s.release();
    } catch (const bt::Error &e) {
        fail(e.code, e.message);
    } catch (const std::exception &e) {
        fail(BT_ERR_PARSE, e.what());
    }
    return nullptr;
}

bt_scene *bt_scene_load(const char *path) {
    if (!path) {
        fail(BT_ERR_INVALID_ARG, "null path");
        return nullptr;
    }
    try {
        std::string text = bt::read_scene_file(path);
        return bt_scene_from_json(text.data(), text.size());
    } catch (const bt::Error &e) {
        fail(e.code, e.message);
    } catch (const std::exception &e) {
        fail(BT_ERR_IO, e.what());
    }
    return nullptr;
}

bt_scene *bt_scene_default(void) {
    std::string text = bt::default_scene_json();
    return bt_scene_from_json(text.data(), text.size());
}

void bt_scene_free(bt_scene *scene) { delete scene; }

int bt_scene_to_json(const bt_scene *scene, char *out, size_t cap) {
    if (!scene) return fail(BT_ERR_INVALID_ARG, "null scene");
    try {
        std::string text = bt::scene_to_pretty_json(scene->scene, scene->source);
        if (out && cap > 0) {
            size_t n = std::min(cap - 1, text.size());
            std::memcpy(out, text.data(), n);
            out[n] = 0;
        }
        return (int)text.size();
    } catch (const bt::Error &e) {
        return fail(e.code, e.message);
    } catch (const std::exception &e) {
        return fail(BT_ERR_PARSE, e.what());
    }
}

int bt_scene_save(const bt_scene *scene, const char *path) {
    if (!scene || !path) return fail(BT_ERR_INVALID_ARG, "null argument");
    try {
        bt::write_text_file(path, bt::scene_to_pretty_json(scene->scene, scene->source));
        return 0;
    } catch (const bt::Error &e) {
        return fail(e.code, e.message);
    } catch (const std::exception &e) {
        return fail(BT_ERR_IO, e.what());
    }
}

int bt_write_png(const char *path, const uint8_t *rgba8, uint32_t width, uint32_t height) {
    if (!path || !rgba8 || width == 0 || height == 0) return fail(BT_ERR_INVALID_ARG, "invalid argument");
    try {
        bt::write_png(path, rgba8, width, height);
        return 0;
    } catch (const bt::Error &e) {
        return fail(e.code, e.message);
    }
}

int bt_write_pfm(const char *path, const float *rgba_host, uint32_t width, uint32_t height, uint32_t samples) {
    if (!path || !rgba_host || width == 0 || height == 0 || samples == 0) return fail(BT_ERR_INVALID_ARG, "invalid argument");
    try {
        bt::write_pfm(path, rgba_host, width, height, samples);
        return 0;
    } catch (const bt::Error &e) {
        return fail(e.code, e.message);
    }
}

int bt_scene_find_by_tag(const bt_scene *scene, const char *tag, uint64_t *object_ref) {
    if (!scene || !tag || !object_ref) return fail(BT_ERR_INVALID_ARG, "null argument");
    for (const bt::Object &o : scene->scene.objects)
        if (o.has_tag && o.tag == tag) {
            *object_ref = o.object_ref;
            return 0;
        }
    return fail(BT_ERR_INVALID_REF, std::string("no object tagged `") + tag + "`");
}

int bt_scene_set_camera_aspect(bt_scene *scene, uint64_t camera_ref, float aspect_ratio) {
    if (!scene) return fail(BT_ERR_INVALID_ARG, "null scene");
    int i = scene->scene.object_index(camera_ref);
    if (i < 0) return fail(BT_ERR_INVALID_REF, "invalid object ref " + std::to_string(camera_ref));
    if (scene->scene.objects[i].kind != bt::OBJ_CAMERA) return fail(BT_ERR_NOT_CAMERA, "expected a camera object");
    scene->scene.objects[i].aspect_ratio = aspect_ratio;   // read at launch time; device tables unaffected
    return 0;
}

int bt_scene_set_lens(bt_scene *scene, const bt_lens *lens) {
    if (!scene) return fail(BT_ERR_INVALID_ARG, "null scene");
    if (!lens) {
        scene->lens_on = false;
        return 0;
    }
    if (!(lens->rs >= 0.0f) || !(lens->step > 0.0f) || !(lens->radius > lens->rs) || lens->max_steps == 0 ||
        lens->max_steps > 0x7fffffffu)
        return fail(BT_ERR_INVALID_ARG, "lens needs rs >= 0, step > 0, radius > rs, max_steps > 0");
    scene->lens = *lens;
    scene->lens_on = true;
    return 0;
}

int bt_scene_object_count(const bt_scene *scene) { return scene ? (int)scene->scene.objects.size() : 0; }
int bt_scene_data_count(const bt_scene *scene) { return scene ? (int)scene->scene.data.size() : 0; }

int bt_scene_export_prims(const bt_scene *scene, float *out, int cap) {
    if (!scene) return fail(BT_ERR_INVALID_ARG, "null scene");
    bt_scene *s = const_cast<bt_scene *>(scene);
    int rc = ensure_flat(s);
    if (rc) return rc;
    const size_t words = sizeof(BtPrim) / 4;
    const int total = (int)(s->flat.prims.size() * words);
    if (out && cap > 0) std::memcpy(out, s->flat.prims.data(), sizeof(float) * (size_t)std::min(cap, total));
    return total;
}

// TEST INFRASTRUCTURE: the sorted view of the table (bt_scene.cpp flatten_scene, bt_device.hpp intersect_sorted) as one
// run of 32-bit words: n_aan[3], n_la, n_other, then the BtRectAAN rows (8 words each), the BtRectLA rows (20 words each)
// and other_rows, each exactly as uploaded
int bt_scene_export_sorted_rows(const bt_scene *scene, uint32_t *out, int cap) {
    if (!scene) return fail(BT_ERR_INVALID_ARG, "null scene");
    bt_scene *s = const_cast<bt_scene *>(scene);
    int rc = ensure_flat(s);
    if (rc) return rc;
    const bt::FlatScene &f = s->flat;
    std::vector<uint32_t> words(5);
    for (int a = 0; a < 3; ++a) words[a] = (uint32_t)f.n_aan[a];
    words[3] = (uint32_t)f.la_rows.size();
    words[4] = (uint32_t)f.other_rows.size();
    auto append = [&words](const void *p, size_t bytes) {
        const size_t at = words.size();
        words.resize(at + bytes / 4);
        if (bytes) std::memcpy(words.data() + at, p, bytes);
    };
    append(f.aan_rows.data(), sizeof(BtRectAAN) * f.aan_rows.size());
    append(f.la_rows.data(), sizeof(BtRectLA) * f.la_rows.size());
    append(f.other_rows.data(), sizeof(int32_t) * f.other_rows.size());
    const int total = (int)words.size();
    if (out && cap > 0) std::memcpy(out, words.data(), sizeof(uint32_t) * (size_t)std::min(cap, total));
    return total;
}

float bt_debug_abs_limit(float limit) { return bt::abs_limit(limit); }

int bt_debug_set_object(bt_scene *scene, uint64_t object_ref, const float *translation, float radius) {
    if (!scene) return fail(BT_ERR_INVALID_ARG, "null scene");
    const int i = scene->scene.object_index(object_ref);
    if (i < 0) return fail(BT_ERR_INVALID_REF, "invalid object ref " + std::to_string(object_ref));
    bt::Object &o = scene->scene.objects[i];
    if (translation) { o.world.t.x = translation[0]; o.world.t.y = translation[1]; o.world.t.z = translation[2]; }
    if (radius > 0.0f && o.kind == bt::OBJ_SPHERE) o.radius = radius;
    scene->flat_valid = false;                            // the tables are flattened and uploaded again by the next render
    return 0;
}

// EXTENSION (bt_view): the camera fields fill_launch puts into BtLaunch, without the tables or a device
int bt_scene_camera_view(const bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                         uint32_t width, uint32_t height, bt_view *out) {
    if (!scene || !config || !render || !out) return fail(BT_ERR_INVALID_ARG, "null argument");
    if (width == 0 || height == 0) return fail(BT_ERR_INVALID_ARG, "zero-sized buffer");
    const int i = scene->scene.object_index(camera_ref);
    if (i < 0) return fail(BT_ERR_INVALID_REF, "invalid object ref " + std::to_string(camera_ref));
    const bt::Object &cam = scene->scene.objects[i];
    if (cam.kind != bt::OBJ_CAMERA) return fail(BT_ERR_NOT_CAMERA, "expected a camera object");
    const BtV3 col[4] = {cam.world.cx, cam.world.cy, cam.world.cz, cam.world.t};
    for (int c = 0; c < 4; ++c) { out->to_world[3 * c] = col[c].x; out->to_world[3 * c + 1] = col[c].y; out->to_world[3 * c + 2] = col[c].z; }
    out->yfov = 2.0f * atan2f(cam.sensor_size, 2.0f * cam.focal_length);  // mod.rs:248
    out->xfov = out->yfov * cam.aspect_ratio;                             // mod.rs:249
    out->clip_min = config->clip_min;
    out->clip_max = config->clip_max;
    out->width = width;
    out->height = height;
    out->subsample_n = render->subsample_n;
    return 0;
}

int bt_scene_set_camera_focus(bt_scene *scene, uint64_t camera_ref, int has_focus, float focus) {
    if (!scene) return fail(BT_ERR_INVALID_ARG, "null scene");
    const int i = scene->scene.object_index(camera_ref);
    if (i < 0) return fail(BT_ERR_INVALID_REF, "invalid object ref " + std::to_string(camera_ref));
    bt::Object &o = scene->scene.objects[i];
    if (o.kind != bt::OBJ_CAMERA) return fail(BT_ERR_NOT_CAMERA, "expected a camera object");
    if (has_focus && !(std::isfinite(focus) && focus > 0.0f)) return fail(BT_ERR_INVALID_ARG, "the focus must be finite and > 0");
    // read at launch time (fill_launch), like the aspect ratio: no table holds it.  The block masks depend on it and their key
    // carries has_focus and focus (bt_cull.hpp MaskKey), so the masks cached under the old focus are not taken again.
    o.has_focus = has_focus != 0;
    o.focus = has_focus ? focus : 0.0f;
    return 0;
}

int bt_scene_query_tables_internal(bt_scene *scene, const BtPrim **prims, const BtQueryRef **refs, int32_t *n_prims) {
    const int rc = ensure_device(scene);
    if (rc) return rc;
    *prims = scene->d_prims.ptr;
    *refs = scene->d_query_refs.ptr;
    *n_prims = (int32_t)scene->flat.prims.size();
    return 0;
}

int bt_scene_set_camera_pose(bt_scene *scene, uint64_t camera_ref, const float *to_world) {
    if (!scene || !to_world) return fail(BT_ERR_INVALID_ARG, "null argument");
    const int i = scene->scene.object_index(camera_ref);
    if (i < 0) return fail(BT_ERR_INVALID_REF, "invalid object ref " + std::to_string(camera_ref));
    bt::Object &o = scene->scene.objects[i];
    if (o.kind != bt::OBJ_CAMERA) return fail(BT_ERR_NOT_CAMERA, "expected a camera object");
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(to_world[k])) return fail(BT_ERR_INVALID_ARG, "non-finite entry in to_world");
    BtV3 *col[4] = {&o.world.cx, &o.world.cy, &o.world.cz, &o.world.t};
    for (int c = 0; c < 4; ++c) { col[c]->x = to_world[3 * c]; col[c]->y = to_world[3 * c + 1]; col[c]->z = to_world[3 * c + 2]; }
    scene->flat_valid = false;                            // as bt_debug_set_object: flattened and uploaded again by the next render
    return 0;
}

// the launch the bt_debug_* mask entry points describe: fill_launch + shard and block shape; returns the number of blocks
static int debug_mask_launch(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                             uint32_t width, uint32_t height, uint32_t slices, uint32_t rank, uint32_t world, BtLaunch &P) {
    if (!scene || !config || !render) return fail(BT_ERR_INVALID_ARG, "null argument");
    if (slices == 0 || slices > 32 || (slices & (slices - 1)) != 0) return fail(BT_ERR_INVALID_ARG, "slices must be 1, 2, 4, ..., 32");
    if (world == 0 || rank >= world) return fail(BT_ERR_INVALID_ARG, "rank/world out of range");
    int rc = ensure_flat(scene);
    if (rc) return rc;
    int output = 0;
    rc = fill_launch(scene, camera_ref, config, render, width, height, 0, P, output);
    if (rc) return rc;
    const uint32_t grid = btplan::shard_launch(P, rank, world, world > 1);
    P.slices = (int32_t)slices;
    const uint64_t n_blocks = (uint64_t)grid * slices;
    if (n_blocks > 0x7fffffffu) return fail(BT_ERR_INVALID_ARG, "too many blocks");
    return (int)n_blocks;
}

int bt_debug_primary_mask(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                          uint32_t width, uint32_t height, uint32_t slices, uint32_t rank, uint32_t world, uint64_t *masks,
                          uint32_t cap) {
    BtLaunch P;
    const int n_blocks = debug_mask_launch(scene, camera_ref, config, render, width, height, slices, rank, world, P);
    if (n_blocks < 0) return n_blocks;
    if (masks && cap > 0) {
        const std::vector<BtSphereRow> rows = sphere_rows_of(scene->flat.prims);
        std::vector<uint64_t> all((size_t)n_blocks, ~0ull);
        if (P.any_rects == 0 && P.any_volumes == 0) bt_primary_masks_host(&P, rows.data(), (uint32_t)n_blocks, all.data());
        std::memcpy(masks, all.data(), sizeof(uint64_t) * (size_t)std::min<uint64_t>(cap, (uint64_t)n_blocks));
    }
    return n_blocks;
}

int bt_debug_block_masks_device(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                                uint32_t width, uint32_t height, uint32_t slices, uint32_t rank, uint32_t world,
                                uint64_t *masks, uint32_t cap) {
    BtLaunch P;
    int n_blocks = debug_mask_launch(scene, camera_ref, config, render, width, height, slices, rank, world, P);
    if (n_blocks < 0) return n_blocks;
    if (!masks || cap == 0) return n_blocks;
    if (P.any_rects || P.any_volumes) return fail(BT_ERR_INVALID_ARG, "the scene does not run the build that reads block masks");
    int rc = ensure_device(scene);
    if (rc) return rc;
    n_blocks = debug_mask_launch(scene, camera_ref, config, render, width, height, slices, rank, world, P);   // (device tables)
    if (n_blocks < 0) return n_blocks;
    uint64_t *d = nullptr;
    BT_HIP(hipMalloc((void **)&d, sizeof(uint64_t) * (size_t)n_blocks));
    hipError_t e = bt_launch_block_masks(&P, (uint32_t)n_blocks, d, nullptr);
    if (e == hipSuccess)
        e = hipMemcpy(masks, d, sizeof(uint64_t) * (size_t)std::min<uint32_t>(cap, (uint32_t)n_blocks), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(BT_ERR_DEVICE, hipGetErrorString(e));
    return n_blocks;
}

int bt_debug_block_order(const uint64_t *masks, uint32_t n_blocks, uint32_t *order_out, uint32_t *header_out) {
    if (!masks || !order_out || !header_out || n_blocks == 0 || n_blocks > 0x7fffffffu) return fail(BT_ERR_INVALID_ARG, "bt_debug_block_order: null argument or no blocks");
    btcull::block_order(masks, n_blocks, order_out, header_out);
    return 0;
}

int bt_debug_block_order_device(const uint64_t *masks, uint32_t n_blocks, uint32_t *order_out, uint32_t *header_out) {
    if (!masks || !order_out || !header_out || n_blocks == 0 || n_blocks > 0x7fffffffu) return fail(BT_ERR_INVALID_ARG, "bt_debug_block_order_device: null argument or no blocks");
    uint64_t *d_masks = nullptr;
    uint32_t *d_out = nullptr;
    hipError_t e = hipMalloc((void **)&d_masks, sizeof(uint64_t) * (size_t)n_blocks);
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, sizeof(uint32_t) * ((size_t)n_blocks + BT_ORDER_HEADER));
    if (e == hipSuccess) e = hipMemcpy(d_masks, masks, sizeof(uint64_t) * (size_t)n_blocks, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = bt_launch_block_order(d_masks, n_blocks, d_out, nullptr);
    if (e == hipSuccess) e = hipMemcpy(header_out, d_out, sizeof(uint32_t) * BT_ORDER_HEADER, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(order_out, d_out + BT_ORDER_HEADER, sizeof(uint32_t) * (size_t)n_blocks, hipMemcpyDeviceToHost);
    if (d_masks) (void)hipFree(d_masks);
    if (d_out) (void)hipFree(d_out);
    if (e != hipSuccess) return fail(BT_ERR_DEVICE, hipGetErrorString(e));
    return 0;
}

int bt_debug_philox_device(const uint32_t *pairs, uint32_t n, uint32_t *out) {
    if (!pairs || !out || n == 0 || n > (1u << 24)) return fail(BT_ERR_INVALID_ARG, "bt_debug_philox_device: null argument, no pairs or more than 2^24");
    uint32_t *d_in = nullptr, *d_out = nullptr;
    hipError_t e = hipMalloc((void **)&d_in, sizeof(uint32_t) * 6 * (size_t)n);
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, sizeof(uint32_t) * 4 * (size_t)n);
    if (e == hipSuccess) e = hipMemcpy(d_in, pairs, sizeof(uint32_t) * 6 * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = bt_launch_philox_test(d_in, n, d_out, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, sizeof(uint32_t) * 4 * (size_t)n, hipMemcpyDeviceToHost);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (e != hipSuccess) return fail(BT_ERR_DEVICE, hipGetErrorString(e));
    return 0;
}

int bt_debug_mask_key(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                      uint32_t width, uint32_t height, uint32_t slices, uint32_t rank, uint32_t world, uint8_t *out,
                      uint32_t cap) {
    BtLaunch P;
    const int n_blocks = debug_mask_launch(scene, camera_ref, config, render, width, height, slices, rank, world, P);
    if (n_blocks < 0) return n_blocks;
    btcull::MaskKey key;
    P.sphere_rows = nullptr;                              // (a device address: not part of what a host-side test compares)
    btcull::mask_key(key, P, (uint32_t)n_blocks, scene->rows_generation, nullptr);
    if (out && cap > 0) std::memcpy(out, &key, std::min<size_t>(cap, sizeof key));
    return (int)sizeof key;
}

int bt_debug_plan_launch(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                         uint32_t width, uint32_t height, uint32_t rank, uint32_t world, int32_t sharded, uint32_t n_cu,
                         int32_t pass_kind, uint32_t guides, uint64_t alloc_limit, bt_stats *out) {
    if (!scene || !config || !render || !out) return fail(BT_ERR_INVALID_ARG, "null argument");
    if (world == 0 || rank >= world) return fail(BT_ERR_INVALID_ARG, "rank/world out of range");
    if (n_cu == 0 || render->samples == 0 || pass_kind < btplan::PLAIN || pass_kind > btplan::ADAPTIVE)
        return fail(BT_ERR_INVALID_ARG, "bt_debug_plan_launch: n_cu and samples must not be 0, pass_kind is 0, 1 or 2");
    int rc = ensure_flat(scene);
    if (rc) return rc;
    BtLaunch P;
    int output = 0;
    rc = fill_launch(scene, camera_ref, config, render, width, height, 0, P, output);
    if (rc) return rc;
    if (pass_kind != btplan::PLAIN && (output != BT_OUTPUT_FULL || scene->lens_on))
        return fail(BT_ERR_INVALID_ARG, "a guided or adaptive pass renders the Full output without the lens");
    btplan::shard_launch(P, rank, world, sharded != 0);
    btplan::Plan plan;
    btplan::Scratch &held = scene->plan_scratch;
    rc = btplan::plan_launch(P, output, scene->flat, scene->tuning, n_cu, pass_kind, guides, held,
                             [&](uint64_t need) -> uint64_t { return alloc_limit == 0 || need <= alloc_limit ? need : 0; }, plan);
    if (rc) return fail(rc, plan.error);
    btplan::plan_stats(P, plan, held, *out);
    out->lens_steps = 0;
    return 0;
}

int bt_render_device(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                     float *rgba_device, uint32_t width, uint32_t height, uint64_t seed, void *stream) {
    return render_common(scene, camera_ref, config, render, rgba_device, width, height, 0, 1, false, seed,
                         (hipStream_t)stream);
}

int bt_render_adaptive_pass_internal(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                                     float *rgba_device, uint32_t width, uint32_t height, uint64_t seed, void *stream,
                                     const uint32_t *tile_active, float *moment) {
    RenderPass pass;
    pass.kind = btplan::ADAPTIVE;
    pass.tile_active = tile_active;
    pass.moment = moment;
    return render_common(scene, camera_ref, config, render, rgba_device, width, height, 0, 1, false, seed, (hipStream_t)stream, pass);
}
int bt_scene_lens_on_internal(const bt_scene *scene) { return scene && scene->lens_on ? 1 : 0; }

int bt_render_guided_device(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                            float *color_device, float *albedo_device, float *normal_device, float *depth_device,
                            uint32_t width, uint32_t height, uint64_t seed, void *stream) {
    // everything that can be refused is refused before the device is touched
    if (!scene || !config || !render || !color_device) return fail(BT_ERR_INVALID_ARG, "null argument");
    const int output = render->has_output ? render->output : config->output;
    if (output != BT_OUTPUT_FULL)
        return fail(BT_ERR_INVALID_ARG, "a guided render is the Full output plus its guides: the effective output must be BT_OUTPUT_FULL");
    float *const frames[4] = {color_device, albedo_device, normal_device, depth_device};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (frames[i] && frames[i] == frames[j]) return fail(BT_ERR_INVALID_ARG, "two frames of a guided render are the same buffer");
    if (scene->lens_on) return fail(BT_ERR_UNSUPPORTED, "the lens extension has no guided builds");
    if (render->samples == 0) return BT_DONE;                          // mod.rs:186-188
    RenderPass pass;
    pass.kind = btplan::GUIDED;
    for (int g = 0; g < 3; ++g) pass.guides[g] = frames[g + 1];
    return render_common(scene, camera_ref, config, render, color_device, width, height, 0, 1, false, seed, (hipStream_t)stream, pass);
}

int bt_render(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
              float *rgba_host, uint32_t width, uint32_t height, uint64_t seed) {
    if (!scene) return fail(BT_ERR_INVALID_ARG, "null scene");
    if (!rgba_host) return fail(BT_ERR_INVALID_ARG, "null buffer");
    if (render && render->samples == 0) return BT_DONE;
    if (width == 0 || height == 0) return fail(BT_ERR_INVALID_ARG, "zero-sized buffer");
    int rc = ensure_device(scene);                        // binds the handle (and its cached frame) to the current device
    if (rc) return rc;
    const size_t bytes = (size_t)width * height * 4 * sizeof(float);
    // the device copy of the caller's buffer lives on the handle: no hipMalloc / hipFree per displayed frame
    const size_t held = scene->d_host_frame.bytes();
    if (held < bytes || held / 4 > bytes) {
        if (scene->d_host_frame.ptr) BT_HIP(hipDeviceSynchronize());
        BT_HIP(scene->d_host_frame.allocate(bytes / sizeof(float)));
    }
    float *d = scene->d_host_frame.ptr;
    BT_HIP(hipMemcpyAsync(d, rgba_host, bytes, hipMemcpyHostToDevice, nullptr));
    rc = bt_render_device(scene, camera_ref, config, render, d, width, height, seed, nullptr);
    if (rc < 0) return rc;
    BT_HIP(hipMemcpy(rgba_host, d, bytes, hipMemcpyDeviceToHost));      // stream-ordered behind the kernel, blocks the host
    return rc;
}

size_t bt_shard_floats(uint32_t width, uint32_t height, uint32_t world) {
    if (world == 0) return 0;
    const size_t per_rank = btplan::tiles_per_rank(btplan::frame_tiles(width, height), world);
    return per_rank * BT_TILE * BT_TILE * 4;
}

int bt_render_shard_device(bt_scene *scene, uint64_t camera_ref, const bt_config *config,
                           const bt_render_config *render, float *shard_device, uint32_t width, uint32_t height,
                           uint32_t rank, uint32_t world, uint64_t seed, void *stream) {
    return render_common(scene, camera_ref, config, render, shard_device, width, height, rank, world, true, seed,
                         (hipStream_t)stream);
}

int bt_unshard_device(const float *gathered_device, float *rgba_device, uint32_t width, uint32_t height, uint32_t world,
                      void *stream) {
    if (!gathered_device || !rgba_device || world == 0 || width == 0 || height == 0)
        return fail(BT_ERR_INVALID_ARG, "invalid argument");
    const uint32_t tiles_x = btplan::tiles_across(width), tiles_y = btplan::tiles_across(height);
    const uint32_t per_rank = btplan::tiles_per_rank(tiles_x * tiles_y, world);
    BT_HIP(bt_launch_unshard(gathered_device, rgba_device, width, height, tiles_x, tiles_y, world, per_rank,
                             (hipStream_t)stream));
    return 0;
}

int bt_preview_device(const float *rgba_device, uint8_t *rgba8_device, uint32_t width, uint32_t height, uint32_t samples,
                      int32_t color_space, void *stream) {
    if (!rgba_device || !rgba8_device || width == 0 || height == 0)
        return fail(BT_ERR_INVALID_ARG, "invalid argument");
    BT_HIP(bt_launch_preview(rgba_device, rgba8_device, width * height, samples, color_space, (hipStream_t)stream));
    return 0;
}

int bt_preview(const float *rgba_host, uint8_t *rgba8_host, uint32_t width, uint32_t height, uint32_t samples,
               int32_t color_space) {
    if (!rgba_host || !rgba8_host || width == 0 || height == 0) return fail(BT_ERR_INVALID_ARG, "invalid argument");
    const size_t n = (size_t)width * height;
    float *d_in = nullptr;
    uint8_t *d_out = nullptr;
    BT_HIP(hipMalloc((void **)&d_in, n * 16));
    hipError_t e = hipMalloc((void **)&d_out, n * 4);
    int rc = 0;
    if (e == hipSuccess) e = hipMemcpy(d_in, rgba_host, n * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) rc = bt_preview_device(d_in, d_out, width, height, samples, color_space, nullptr);
    if (e == hipSuccess && rc == 0) e = hipMemcpy(rgba8_host, d_out, n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (e != hipSuccess) return fail(BT_ERR_DEVICE, hipGetErrorString(e));
    return rc;
}

int bt_scene_trim(bt_scene *scene) {
    if (!scene) return fail(BT_ERR_INVALID_ARG, "null scene");
    scene->plan_scratch = btplan::Scratch{};
    if (scene->device < 0 || (!scene->d_scratch.ptr && !scene->d_host_frame.ptr && !scene->d_block_masks.ptr)) return 0;
    int cur = -1;
    BT_HIP(hipGetDevice(&cur));
    if (cur != scene->device) BT_HIP(hipSetDevice(scene->device));
    BT_HIP(hipDeviceSynchronize());                       // launches that still read the scratch / the cached frame
    scene->release_buffers();
    if (cur != scene->device) BT_HIP(hipSetDevice(cur));
    return 0;
}

int bt_scene_last_stats(bt_scene *scene, bt_stats *out) {
    if (!scene || !out) return fail(BT_ERR_INVALID_ARG, "null argument");
    if (scene->stats_pending) {
        BT_HIP(hipEventSynchronize(scene->ev_stop));
        unsigned long long c[16] = {0, 0};
        BT_HIP(hipMemcpy(c, scene->d_counters + (size_t)scene->last_slot * 16, sizeof c, hipMemcpyDeviceToHost));
#ifdef BT_LANESTAT
        // developer build (-DBT_LANESTAT): what the lanes of a wave do per iteration, see bt_kernels.hip
        if (c[2]) {
            const double it = (double)c[2] * 64.0;
            fprintf(stderr, "[bt lanes] wave-iterations %llu; of 64 lanes per iteration: trace %.1f%% | camera %.1f%% diffuse %.1f%% metallic %.1f%% glass %.1f%% volume %.1f%% | waiting for phase %.1f%% | left the loop %.1f%%\n",
                    c[2], 100.0 * c[3] / it, 100.0 * c[4] / it, 100.0 * c[5] / it, 100.0 * c[6] / it, 100.0 * c[7] / it,
                    100.0 * c[8] / it, 100.0 * c[9] / it, 100.0 * c[10] / it);
        }
#elif defined(BT_PROFILE)
        // developer build (-DBT_PROFILE): wave cycles per section of the render loop, see bt_kernels.hip
        {
            unsigned long long tot = 0;
            for (int i = 2; i < BT_N_COUNTERS; ++i) tot += c[i];
            fprintf(stderr, "[bt profile] section share of wave cycles:");
            for (int i = 2; i < BT_N_COUNTERS; ++i) fprintf(stderr, " s%d=%.1f%%", i - 2, tot ? 100.0 * (double)c[i] / (double)tot : 0.0);
            fprintf(stderr, "\n");
        }
#endif
        float ms = 0.0f;
        BT_HIP(hipEventElapsedTime(&ms, scene->ev_start, scene->ev_stop));
        scene->last.segments = c[0];
        scene->last.lens_steps = c[1];
        scene->last.kernel_ms = ms;
        scene->stats_pending = false;
    }
    *out = scene->last;
    return 0;
}

} // extern "C"
