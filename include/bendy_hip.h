/*
 * bendy_hip.h -- C ABI of libbendy_hip.so, the MI355X (gfx950) implementation of
 * bendy-tracer's per-pixel / per-sample hot path.
 *
 * The reference (soycan-sim/bendy-tracer @ v1) has no FFI surface; its boundary is
 * the Rust library API that src/main.rs uses.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference tree).
 * INTEGRATION.md shows the Rust `extern "C"` binding a maintainer would add.
 *
 * Conventions: plain pointers and sizes only; no exceptions cross the ABI; every
 * function that can fail returns a negative bt_status and records a message that
 * bt_last_error() returns (thread-local).  A bt_scene handle is not thread-safe
 * for concurrent bt_render* calls (same as `&mut Buffer` in the reference).
 */
#ifndef BENDY_HIP_H
#define BENDY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* tracer/mod.rs:159-163 `Status` (>= 0) and error codes (< 0; the reference panics instead). */
typedef enum {
    BT_DONE = 0,               /* Status::Done: samples == 0 (mod.rs:186-188) */
    BT_IN_PROGRESS = 1,        /* Status::InProgress (mod.rs:201) */
    BT_ERR_INVALID_ARG = -1,
    BT_ERR_IO = -2,            /* file missing / gzip error (main.rs:93-102) */
    BT_ERR_PARSE = -3,         /* malformed JSON / unexpected schema (serde error in the reference) */
    BT_ERR_INVALID_REF = -4,   /* "invalid object ref" / "invalid data ref" (scene/mod.rs:132,136) */
    BT_ERR_NOT_CAMERA = -5,    /* "expected a camera object" (tracer/mod.rs:246) */
    BT_ERR_NOT_MATERIAL = -6,  /* "expected material data" / "expected volume data" (mod.rs:464,499) */
    BT_ERR_NO_LIGHT = -7,      /* Diffuse material but no LIGHT object: Uniform::new(0,0) panics (material.rs:112) */
    BT_ERR_DEVICE = -8,        /* HIP runtime error / no gfx950 device */
    BT_ERR_UNSUPPORTED = -9
} bt_status;

/* tracer/mod.rs:108-115 `Output` */
typedef enum { BT_OUTPUT_FULL = 0, BT_OUTPUT_ALBEDO = 1, BT_OUTPUT_NORMAL = 2, BT_OUTPUT_DEPTH = 3 } bt_output;

/* tracer/buffer.rs:11-17 `ColorSpace` */
typedef enum { BT_COLOR_NONE = 0, BT_COLOR_NORMAL = 1, BT_COLOR_LINEAR = 2, BT_COLOR_SRGB = 3 } bt_color_space;

/* tracer/mod.rs:16-26 `Config`; bt_config_default() = Config::DEFAULT (:29-38). */
typedef struct {
    uint32_t max_bounces;
    uint32_t max_volume_bounces;
    float clip_min;
    float clip_max;
    float volume_step;
    uint32_t chunks_x;         /* kept for API fidelity; the GPU grid does its own tiling */
    uint32_t chunks_y;
    int32_t output;            /* bt_output */
} bt_config;

/* tracer/mod.rs:117-125 `RenderConfig` (Option<T> -> has_* flag + value);
 * bt_render_config_default() = RenderConfig::DEFAULT (:128-135). */
typedef struct {
    uint32_t subsample_n;      /* Subsample: 0 or 1 = None, n >= 2 = Subpixel(n) (:47-52, main.rs:234-237) */
    uint32_t samples;
    int32_t has_output;
    int32_t output;
    int32_t has_max_bounces;
    uint32_t max_bounces;
    int32_t has_max_volume_bounces;
    uint32_t max_volume_bounces; /* accepted but ignored, exactly like the reference (quirk Q1, mod.rs:224) */
    int32_t has_volume_step;
    float volume_step;
    /* Not in the reference (it seeds from OS entropy, mod.rs:239-242): index of this
     * call's first sample, so that k progressive calls of 1 sample equal one call of
     * k samples bit for bit.  Callers normally pass Buffer::samples() / n^2. */
    uint32_t sample_base;
} bt_render_config;

/* Work counters of the last render on a scene handle (for the roofline model). */
typedef struct {
    uint64_t samples;          /* rays per pixel * pixels rendered by this rank */
    uint64_t segments;         /* try_hit / try_hit_volume calls (mod.rs:389-427) */
    uint64_t pixels;
    float kernel_ms;           /* HIP-event time of the render kernel(s), 0 if not measured */
    uint64_t lens_steps;       /* RK4 steps taken by the lens extension (0 when it is off) */
    uint32_t slices;           /* S of the last launch: pixel blocks of 256/S pixels whose samples are dealt to the lanes of a
                                * workgroup through a queue; DESIGN.md 5.3 */
    uint32_t launches;         /* kernel launches the render was split into (deep renders under the scratch cap) */
    uint64_t scratch_bytes;    /* HBM the handle holds for parked sample values after this render */
    uint64_t parked_bytes;     /* bytes of sample values the render parked in HBM (12 per sample, edge tiles padded;
                                * a guided render: + 12 / 12 / 4 per guide) */
    uint32_t workgroups;       /* workgroups of the last launch */
    uint32_t packed;           /* 1 / 2: the last launch was packed (bt_tuning.packed; 2 = with the compacting drain): `workgroups` = the
                                * GPU's workgroup slots, each owning every workgroups-th pixel block behind one queue */
} bt_stats;

/* Launch-shape knobs of a scene handle.  Every field's zero / negative value means "let the library decide" (what
 * bt_tuning_default() fills in); the library itself never reads environment variables.  Tests and the A/B tools under
 * tools/ set these to pin a shape; none of them can change a pixel (tests/test_gpu_parity.py renders every setting). */
typedef struct {
    uint32_t slices;           /* 0 = auto; 1, 2, 4, 8, 16, 32: pixel blocks of 256 / slices pixels */
    int32_t phase_vote;        /* -1 = auto; 0 = off; n = longest wait of the phase vote in iterations */
    uint64_t scratch_cap_bytes;/* 0 = the default 2 GiB: most parked sample values per launch; deeper renders are split into
                                * several launches over consecutive sample ranges */
    int32_t packed;            /* -1 = auto; 0 = one pixel block per workgroup; 1 / 2 = packed launch where one fits: one workgroup per
                                * workgroup slot of the GPU, each owning every n-th pixel block behind one queue --
                                * 2 (what auto uses): its drain compacts the paths in flight into fewer waves through LDS records */
    int32_t reserved;
} bt_tuning;

/* EXTENSION -- NOT IN THE REFERENCE.  bendy-tracer v1 traces straight rays only (`Ray::at` is
 * origin + t * direction, tracer/ray.rs:115-117); "gravitational lensing" exists in its README as an
 * aspiration.  This optional mode (off unless set) bends every non-marching path segment around one point
 * mass: inside `radius` the photon follows the Schwarzschild null geodesic, integrated with fixed-step RK4
 * (x'' = -1.5 rs h^2 x / r^5, h = |x x v|), and each step's chord is intersected like a volume-march step;
 * outside `radius` rays are straight; r <= rs swallows the path (black).  Light-sampling pdfs
 * (material.rs:313-316) still assume straight visibility.  There is no reference behaviour to match:
 * validation is analytic (weak-field deflection 2 rs / b, capture below b = 3 sqrt(3)/2 rs) plus GPU == CPU
 * oracle; with the lens unset every code path and every pixel is exactly what it is without this extension. */
typedef struct {
    float centre[3];
    float rs;                  /* Schwarzschild radius, scene units */
    float step;                /* RK4 step (affine length) */
    float radius;              /* sphere of influence */
    uint32_t max_steps;        /* RK4 steps per path segment before the segment is abandoned as a miss */
} bt_lens;

typedef struct bt_scene bt_scene; /* opaque; replaces `Scene` (scene/mod.rs:84-90) */

void bt_config_default(bt_config *out);                 /* Config::default(), mod.rs:41-45 */
void bt_render_config_default(bt_render_config *out);   /* RenderConfig::default(), mod.rs:153-157 */
const char *bt_last_error(void);
int bt_last_error_code(void);      /* bt_status of the last failure on this thread (for NULL-returning constructors) */
const char *bt_version(void);

/* --- Scene: serde_json::from_reader(GzDecoder) in main.rs:93-102 ------------------- */
/* `path` ends in .gz -> gzip, else plain JSON (main.rs:97-102).  NULL on error. */
bt_scene *bt_scene_load(const char *path);
/* serde_json::from_slice on an in-memory, already decompressed document. */
bt_scene *bt_scene_from_json(const char *json, size_t len);
/* The scene main.rs builds when the --scene file does not exist (main.rs:107-214). */
bt_scene *bt_scene_default(void);
void bt_scene_free(bt_scene *scene);
/* serde_json::to_writer_pretty(&scene) (main.rs:299-313): writes up to cap-1 bytes + NUL into `out`
 * (may be NULL) and returns the full length.  bt_scene_save gzips when `path` ends in .gz. */
int bt_scene_to_json(const bt_scene *scene, char *out, size_t cap);
int bt_scene_save(const bt_scene *scene, const char *path);
/* buffer.preview().save(path) (main.rs:275-298): RGBA8 PNG. */
int bt_write_png(const char *path, const uint8_t *rgba8, uint32_t width, uint32_t height);
/* Scene::find_by_tag (scene/mod.rs:124-129).  Writes the ObjectRef; returns 0, or
 * BT_ERR_INVALID_REF if no object carries the tag.  When several objects share a tag
 * the lowest ObjectRef wins (the reference's hash-map order is unspecified). */
int bt_scene_find_by_tag(const bt_scene *scene, const char *tag, uint64_t *object_ref);
/* object.as_camera_mut().unwrap().aspect_ratio = a (main.rs:218-223, quirk Q12). */
int bt_scene_set_camera_aspect(bt_scene *scene, uint64_t camera_ref, float aspect_ratio);
/* Lens extension (see bt_lens): NULL switches it off again. */
int bt_scene_set_lens(bt_scene *scene, const bt_lens *lens);
int bt_scene_object_count(const bt_scene *scene);
int bt_scene_data_count(const bt_scene *scene);
/* Flattened primitive table as uploaded to the GPU, for loader cross-checks:
 * writes up to `cap` floats, returns the number available. */
int bt_scene_export_prims(const bt_scene *scene, float *out, int cap);
/* For tests: the sorted view of that table which rect scenes without volumes are intersected through, as
 * uploaded, in 32-bit words: n_aan[3] (x-, y-, z-normal rows), n_la, n_other, then the axis-aligned rows (8 words each:
 * it_a, it_b, lim_a, lim_b, t_w, sgn_mask, prio, pad), the rows of rects with axis-aligned local axes (20 words each:
 * n[3], first_of_normal, t[3], prio, a_x[2], a_y[2], a_z[2], a_w[2], lim[2], pad[2]) and the indices of every other row
 * of the primitive table.  Writes up to `cap` words (out may be NULL), returns the number available. */
int bt_scene_export_sorted_rows(const bt_scene *scene, uint32_t *out, int cap);
/* For tests: the limit those rows carry for a squared half extent `limit` -- the largest s with fl(s * s) <= limit, so
 * that Rect::contains_point's `x * x <= limit` (rect.rs:74-80) is |x| <= s; -1 for a negative or NaN limit. */
float bt_debug_abs_limit(float limit);
/* For tests: the per-block sphere masks of the sphere-only build without volumes, computed on the host
 * by the mask kernel's own code.  Blocks of a launch with `slices` (1, 2, 4, ..., 32) blocks per 16x16 tile, in launch order:
 * tile-major over the frame, or over rank `rank`'s tiles when world > 1.  Bit i set = sphere row i may be hit by a primary
 * ray of the block; a block with no bit set traces nothing.  Writes up to `cap` masks (masks may be NULL) and returns the
 * number of blocks; every bit is set for scenes that do not run that build. */
int bt_debug_primary_mask(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                          uint32_t width, uint32_t height, uint32_t slices, uint32_t rank, uint32_t world, uint64_t *masks,
                          uint32_t cap);

/* For tests of what a handle keeps between renders: moves an object (translation = 3 floats of transform_world, or NULL)
 * and / or resizes a sphere (radius > 0) IN PLACE; the next render flattens and uploads the tables again.  The JSON that
 * bt_scene_save / bt_scene_to_json write is not updated. */
int bt_debug_set_object(bt_scene *scene, uint64_t object_ref, const float *translation, float radius);
/* For tests: the same masks as bt_block_mask_kernel writes them on the current device (the kernel the render launches read
 * their masks from), copied back.  Same arguments and return value as bt_debug_primary_mask; BT_ERR_INVALID_ARG for a scene
 * that does not run that build. */
int bt_debug_block_masks_device(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                                uint32_t width, uint32_t height, uint32_t slices, uint32_t rank, uint32_t world,
                                uint64_t *masks, uint32_t cap);
/* For tests: the order in which a launch takes its blocks, from their masks (bt_debug_primary_mask's): order_out[n_blocks] =
 * the indices of the non-zero masks, ascending, then those of the zero masks, ascending; header_out[2] = the two counts.
 * Computed on the host by the function that defines the result.  Returns 0. */
int bt_debug_block_order(const uint64_t *masks, uint32_t n_blocks, uint32_t *order_out, uint32_t *header_out);
/* For tests: the same, written by the kernel the renders get their order from, on the current device, and copied back. */
int bt_debug_block_order_device(const uint64_t *masks, uint32_t n_blocks, uint32_t *order_out, uint32_t *header_out);
/* For tests: the device's Philox4x32-10 in the form the sphere-only render builds run it (wave-uniform key)
 * on the current device: pairs[6 * i ...] = counter words c0 .. c3, key words k0, k1 of pair i; out[4 * i ...] = its four
 * words.  Each wave takes 64 pairs and goes through their keys one at a time, so that the key is wave-uniform as a launch's
 * seed is.  Returns 0. */
int bt_debug_philox_device(const uint32_t *pairs, uint32_t n, uint32_t *out);
/* For tests: the bytes of the key under which a handle keeps such a launch's masks between renders (stream = NULL, no
 * device address): any input the masks depend on must change them.  Writes up to `cap` bytes, returns the key's size. */
int bt_debug_mask_key(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                      uint32_t width, uint32_t height, uint32_t slices, uint32_t rank, uint32_t world, uint8_t *out,
                      uint32_t cap);

/* For tests of the launch planner, on a machine without a GPU: what a render of these arguments on a device
 * of `n_cu` compute units would launch.  pass_kind: 0 plain, 1 guided with `guides` = bit 0 albedo | bit 1 normal | bit 2
 * depth present, 2 adaptive.  No device is touched: allocations of more than `alloc_limit` bytes fail (0 = none fails).
 * Fills the launch-shape fields of `out` (slices, launches, packed, workgroups, scratch_bytes, parked_bytes, pixels,
 * samples; the others 0) and returns 0, or the bt_status the render would fail with.  The first plan on a handle starts
 * from an empty scratch; later ones from what the earlier ones left, as renders do (bt_scene_trim empties it). */
int bt_debug_plan_launch(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                         uint32_t width, uint32_t height, uint32_t rank, uint32_t world, int32_t sharded, uint32_t n_cu,
                         int32_t pass_kind, uint32_t guides, uint64_t alloc_limit, bt_stats *out);

/* --- Tracer::render (tracer/mod.rs:179-202) ----------------------------------------
 * Adds `samples * n^2` radiance samples per pixel into the RGB channels of `rgba`
 * (row-major, 4 floats per pixel, alpha untouched: buffer.rs:159-178).  The caller
 * tracks Buffer::samples += samples * n^2 (mod.rs:199).  `seed` replaces
 * SmallRng::from_entropy() (mod.rs:239-242).  Returns BT_DONE when samples == 0,
 * BT_IN_PROGRESS otherwise, < 0 on error.  Nothing is retained after return. */

/* Host buffer: copies H2D into a device frame cached on the scene handle, renders on the current device, copies D2H
 * (two PCIe transfers of w*h*16 bytes per call).  A caller that renders once per displayed frame (main.rs:245-254)
 * should keep the frame on the device and use bt_render_device + bt_preview_device instead. */
int bt_render(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
              float *rgba_host, uint32_t width, uint32_t height, uint64_t seed);

/* Device-resident buffer; `stream` is a hipStream_t (NULL = default stream).  The call
 * enqueues work and returns without synchronising. */
int bt_render_device(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                     float *rgba_device, uint32_t width, uint32_t height, uint64_t seed, void *stream);

/* EXTENSION -- NOT IN THE REFERENCE.  One pass of Tracer::render that adds the colour samples to
 * `color_device` and, from the same paths, the BT_OUTPUT_ALBEDO / _NORMAL / _DEPTH values to the
 * guide frames (any of them may be NULL).  Every frame ends up bit-identical to what
 * bt_render_device writes with the same arguments and the corresponding output: the reference fills
 * ColorData.albedo / normal / depth in the same recursion that produces the colour (mod.rs:304-315),
 * this entry point keeps all four -- what bt_denoise_device wants per displayed frame.
 * Checked before the device is touched, in this order: NULL scene / config / render / colour and an
 * effective output (render.output if has_output, else config.output) other than BT_OUTPUT_FULL ->
 * BT_ERR_INVALID_ARG; two of the four frames being the same pointer -> BT_ERR_INVALID_ARG; a lens
 * set on the scene -> BT_ERR_UNSUPPORTED; samples == 0 -> BT_DONE.  With all three guides NULL it is
 * bt_render_device.  A guided sample parks 12 + 12 (albedo) + 12 (normal) + 4 (depth) bytes in the
 * handle's scratch, so a deep render is split into more launches than the plain one
 * (bt_tuning.scratch_cap_bytes); bt_stats.parked_bytes counts what was parked.
 * Not provided: a host-buffer variant, a sharded variant and builds for the lens extension;
 * bt_denoise* is unchanged. */
int bt_render_guided_device(bt_scene *scene, uint64_t camera_ref, const bt_config *config,
                            const bt_render_config *render, float *color_device, float *albedo_device,
                            float *normal_device, float *depth_device, uint32_t width, uint32_t height,
                            uint64_t seed, void *stream);

/* --- Multi-GPU pixel-tile sharding (new; the reference's only parallelism is rayon
 * tiles inside one process, tracer/mod.rs:190-197) ---------------------------------
 * The frame is cut into BT_TILE x BT_TILE pixel tiles, numbered row-major; rank r of
 * `world` owns tiles r, r+world, r+2*world, ...  A shard holds the rank's tiles
 * back to back, each tile BT_TILE*BT_TILE*4 floats (padded tiles included), so every
 * rank's shard has bt_shard_floats() elements and an all-gather concatenates them. */
#define BT_TILE 16
size_t bt_shard_floats(uint32_t width, uint32_t height, uint32_t world);
/* Renders this rank's tiles into `shard_device`, which must hold the rank's
 * running sums in shard layout (zero + alpha 1 for a fresh frame). */
int bt_render_shard_device(bt_scene *scene, uint64_t camera_ref, const bt_config *config,
                           const bt_render_config *render, float *shard_device, uint32_t width, uint32_t height,
                           uint32_t rank, uint32_t world, uint64_t seed, void *stream);
/* gathered = `world` shards back to back (the all-gather result) -> row-major frame. */
int bt_unshard_device(const float *gathered_device, float *rgba_device, uint32_t width, uint32_t height,
                      uint32_t world, void *stream);

/* The exchange step: one RCCL all-gather over xGMI of every rank's shard, one process per GPU.  RCCL is bound at run
 * time (librccl.so.1; a copy the process already holds, e.g. PyTorch's, is shared).  Rank 0 obtains a unique id and
 * hands it to the other ranks by any host-side channel (a file, a socket, MPI); bt_comm_init is collective. */
#define BT_COMM_ID_BYTES 128
typedef struct bt_comm bt_comm;
/* ncclGetUniqueId: writes BT_COMM_ID_BYTES bytes, returns that count, < 0 on error. */
int bt_comm_unique_id(void *id_out, size_t cap);
/* ncclCommInitRank on the current device.  NULL on error (bt_last_error). */
bt_comm *bt_comm_init(uint32_t rank, uint32_t world, const void *unique_id, size_t id_bytes);
void bt_comm_free(bt_comm *comm);
int bt_comm_rank(const bt_comm *comm);
int bt_comm_world(const bt_comm *comm);
/* ncclAllGather(shard -> gathered, bt_shard_floats(width, height, world) floats per rank) on `stream`. */
int bt_allgather_shards_device(bt_comm *comm, const float *shard_device, float *gathered_device, uint32_t width,
                               uint32_t height, void *stream);
/* All-gather + bt_unshard_device: every rank ends up with the row-major frame of running sums in `rgba_device`
 * (north_star: "RCCL all-gather over xGMI of the final framebuffer").  `gathered_device` is world * shard floats of
 * staging the caller owns. */
int bt_exchange_frame_device(bt_comm *comm, const float *shard_device, float *gathered_device, float *rgba_device,
                             uint32_t width, uint32_t height, void *stream);

/* --- Buffer::preview (tracer/buffer.rs:117-138): sum/samples -> colour space -> RGBA8 */
int bt_preview_device(const float *rgba_device, uint8_t *rgba8_device, uint32_t width, uint32_t height,
                      uint32_t samples, int32_t color_space, void *stream);
int bt_preview(const float *rgba_host, uint8_t *rgba8_host, uint32_t width, uint32_t height, uint32_t samples,
               int32_t color_space);

/* --- EXTENSION -- NOT IN THE REFERENCE: AOV-guided a-trous denoiser ------------------------------
 * bendy-tracer v1 has no denoiser.  This one is off unless called, makes no parity claim and changes no render.
 * Edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) on the albedo-demodulated colour (as in SVGF),
 * guided by the BT_OUTPUT_ALBEDO / _NORMAL / _DEPTH sums of the same frame.  Inputs are RGBA32F running sums, each
 * with its own sample count; albedo, normal and depth may be NULL (that guide's weight is then 1).  `out` receives
 * the MEAN (preview it with samples = 1): out.rgb = filtered colour, out.a = the colour buffer's alpha;
 * levels == 0 writes the plain mean.  `out` must not be one of the inputs.  Invalid arguments are rejected before
 * the device is touched (BT_ERR_INVALID_ARG); a valid call without a device returns BT_ERR_DEVICE. */
typedef struct {
    uint32_t levels;           /* a-trous levels (steps 1, 2, 4, ...), 0 .. 10 */
    float sigma_color;         /* > 0: colour edge stop, exp(-|e_p - e_q|^2 4^i / sigma_color^2) at level i */
    float sigma_normal;        /* >= 0: normal edge stop, max(0, n_p . n_q)^sigma_normal */
    float sigma_depth;         /* > 0: depth edge stop, relative to the centre's depth */
    float eps_albedo;          /* >= 0: albedo channels <= eps_albedo are not demodulated */
} bt_denoise_params;
typedef struct bt_denoiser bt_denoiser;   /* owns the scratch (48 B per pixel); grows on demand; one stream at a time */
void bt_denoise_params_default(bt_denoise_params *out);
bt_denoiser *bt_denoiser_new(void);
void bt_denoiser_free(bt_denoiser *d);
/* Device-resident buffers (w * h * 4 floats each); `stream` is a hipStream_t (NULL = default stream).  Enqueues
 * levels + 1 kernels and returns without synchronising.  params == NULL: bt_denoise_params_default. */
int bt_denoise_device(bt_denoiser *d, const float *color, uint32_t color_samples,
                      const float *albedo, uint32_t albedo_samples,
                      const float *normal, uint32_t normal_samples,
                      const float *depth, uint32_t depth_samples,
                      float *out, uint32_t width, uint32_t height, const bt_denoise_params *params, void *stream);
/* Host buffers: copied through the device like bt_render (device staging kept on the handle); blocks until `out` is written. */
int bt_denoise(bt_denoiser *d, const float *color, uint32_t color_samples,
               const float *albedo, uint32_t albedo_samples,
               const float *normal, uint32_t normal_samples,
               const float *depth, uint32_t depth_samples,
               float *out, uint32_t width, uint32_t height, const bt_denoise_params *params);

/* --- EXTENSION -- NOT IN THE REFERENCE: variance-driven adaptive sampling -------------------------
 * bendy-tracer v1 spends the same number of samples on every pixel.  This mode is off unless called and changes no
 * other entry point.  A bt_adaptive handle keeps, for one frame size, a per-pixel second moment (the running sum of
 * the squared Rec. 709 luminance of the pixel's samples, 4 B per pixel) and per 16x16 tile a sample count, an error
 * estimate and an activity flag.  One pass (bt_render_adaptive_device) adds render.samples * n^2 samples per pixel to
 * the tiles that are still active -- the paths, Philox blocks and additions of bt_render_device, so a tile with
 * count c holds bit for bit what bt_render_device gives its pixels for the sample indices [0, c / n^2) -- and then
 * re-estimates every active tile.  With T = samples * n^2, c = the tile's count after the pass, (r, g, b) a pixel's
 * colour sum and M its moment, all in float32:
 *     S = (0.2126 r + 0.7152 g) + 0.0722 b;  mu = S / c;  var = max(0, M / c - mu * mu);
 *     e_p = sqrt(var / c) / (mu + eps), a non-finite e_p counting as 0;
 *     e_t = the mean of e_p over the tile's pixels inside the frame;
 *     the tile stops when c >= max_samples, or when c >= min_samples and e_t <= threshold; it never starts again.
 * Counts are in samples per pixel (n^2 per subsampled sample), as Buffer::samples is. */
typedef struct {
    float threshold;           /* >= 0, finite: a tile stops once its relative standard error e_t is at or below it */
    uint32_t min_samples;      /* samples per pixel every tile gets before it may stop on its error */
    uint32_t max_samples;      /* >= min_samples: samples per pixel at which a tile stops whatever its error */
    float eps;                 /* added to the mean luminance in e_p's denominator */
} bt_adaptive_params;
typedef struct {
    uint32_t active_tiles;     /* tiles the next pass would sample */
    uint32_t tiles;
    uint32_t min_count, max_count;   /* smallest / largest per-tile count */
    uint64_t pixel_samples;    /* samples taken so far, summed over the frame's pixels */
    uint32_t passes;           /* passes since bt_adaptive_reset */
    uint32_t reserved;
} bt_adaptive_stats;
typedef struct bt_adaptive bt_adaptive;   /* owns moment plane, counts, flags, errors; one frame size, one stream at a time */
void bt_adaptive_params_default(bt_adaptive_params *out);
/* No device work happens here: the buffers are allocated by the first pass, on the device current then.  NULL for a
 * zero-sized frame. */
bt_adaptive *bt_adaptive_new(uint32_t width, uint32_t height);
void bt_adaptive_free(bt_adaptive *a);
/* Zero moments, counts and errors, every tile active, next sample index 0, the pass size forgotten. */
int bt_adaptive_reset(bt_adaptive *a);
/* One asynchronous pass on `stream` into `rgba_device` (the frame of running sums, row-major RGBA32F, which must hold
 * the sums of the handle's earlier passes since the reset -- zero + alpha for a fresh frame).  render.sample_base is
 * ignored: the handle's next sample index is used.  Never a packed launch; shares the scene handle's scratch, split
 * launches and pinned slices with bt_render_device.  Checked before the device is touched, in this order: NULL scene /
 * config / render / adaptive / params / rgba -> BT_ERR_INVALID_ARG; an effective output other than BT_OUTPUT_FULL ->
 * BT_ERR_INVALID_ARG; width, height other than the handle's -> BT_ERR_INVALID_ARG; threshold negative or not finite
 * -> BT_ERR_INVALID_ARG; min_samples > max_samples -> BT_ERR_INVALID_ARG; samples or subsample_n other than those
 * of the handle's earlier passes since the reset -> BT_ERR_INVALID_ARG; a lens set on the scene -> BT_ERR_UNSUPPORTED;
 * samples == 0 -> BT_DONE.  Returns BT_DONE as well (nothing is launched) once a poll has found no tile active, else
 * BT_IN_PROGRESS.  bt_scene_last_stats afterwards: `samples` counts every tile as if it were active.
 * Not provided: guided, sharded, host-buffer, lens and packed variants, and a finer granularity than the tile. */
int bt_render_adaptive_device(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                              bt_adaptive *adaptive, const bt_adaptive_params *params, float *rgba_device, uint32_t width,
                              uint32_t height, uint64_t seed, void *stream);
/* Waits for the stream of the last pass; BT_DONE when no tile is active any more, else BT_IN_PROGRESS.  `out` may be NULL. */
int bt_adaptive_poll(bt_adaptive *a, bt_adaptive_stats *out);
/* Per-tile counts / error estimates (tiles row-major, tiles_x = ceil(width / 16)) and, for tests, the per-pixel moment
 * plane (row-major): n == 0 returns the number of elements, else up to n are copied to `host` (synchronises) and the
 * number copied is returned. */
int bt_adaptive_counts(bt_adaptive *a, uint32_t *host, uint32_t n);
int bt_adaptive_errors(bt_adaptive *a, float *host, uint32_t n);
int bt_debug_adaptive_moments(bt_adaptive *a, float *host, uint32_t n);
/* out.rgb = rgba.rgb * (1 / the pixel's tile's count), 0 for a count of 0; out.a = rgba.a: the MEAN, to be previewed
 * with samples = 1 or handed to bt_denoise_device with color_samples = 1.  `out` must not be `rgba`. */
int bt_adaptive_resolve_device(bt_adaptive *a, const float *rgba_device, float *out_device, void *stream);

/* --- EXTENSION -- NOT IN THE REFERENCE: temporal accumulation with reprojection --------------------
 * bendy-tracer v1 throws every sample of a frame buffer away when the camera moves (Buffer::clear, main.rs:325).  This
 * stage is off unless called, makes no parity claim and changes no render.  It keeps the previous frame's accumulated
 * colour and guides, finds where each pixel of the new frame was in the old one and blends (the temporal stage of SVGF,
 * Schied et al. 2017, without its variance history).  The world is assumed static: only the camera moves.
 *
 * bt_view is the camera as data: what a render with the same arguments puts into its launch. */
typedef struct {
    float to_world[12];        /* the camera's transform_world: columns x, y, z, then the translation */
    float yfov, xfov;          /* 2 atan2(sensor, 2 focal) and yfov * aspect (mod.rs:248-249) */
    float clip_min, clip_max;
    uint32_t width, height, subsample_n;   /* subsample_n as in bt_render_config: 0 / 1 = None */
} bt_view;
/* Touches no device.  BT_ERR_INVALID_REF / BT_ERR_NOT_CAMERA as renders do; NULL arguments or a zero-sized frame ->
 * BT_ERR_INVALID_ARG. */
int bt_scene_camera_view(const bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render,
                         uint32_t width, uint32_t height, bt_view *out);
/* Replaces the camera's transform_world IN PLACE (12 floats, laid out as bt_view.to_world); the next render flattens and
 * uploads the tables again, as after bt_debug_set_object.  BT_ERR_NOT_CAMERA for another kind of object,
 * BT_ERR_INVALID_ARG for a non-finite entry.  The JSON that bt_scene_save / bt_scene_to_json write is not updated. */
int bt_scene_set_camera_pose(bt_scene *scene, uint64_t camera_ref, const float *to_world);

typedef struct {
    float alpha_min;           /* [0, 1]: floor of the blend weight of the new frame */
    float max_history;         /* >= 1, finite: the history length (in samples per pixel) is clamped to this */
    float depth_tolerance;     /* >= 0: a tap passes if |z' - z_q| <= depth_tolerance * z' */
    float normal_min;          /* [-1, 1]: a tap passes if n_p . n_q >= normal_min */
} bt_temporal_params;
typedef struct bt_temporal bt_temporal;   /* owns two history and two guide planes (64 B per pixel) and the previous view;
                                           * one frame size, one stream at a time */
void bt_temporal_params_default(bt_temporal_params *out);
/* No device work happens here: the planes are allocated by the first accumulate, on the device current then.  NULL for a
 * zero-sized frame. */
bt_temporal *bt_temporal_new(uint32_t width, uint32_t height);
void bt_temporal_free(bt_temporal *t);
/* Forgets the history and the previous view: the next accumulate writes the frame's own mean. */
int bt_temporal_reset(bt_temporal *t);
/* One kernel on `stream`; returns without synchronising.  The inputs are RGBA32F running sums of THIS frame alone (what
 * bt_render_guided_device wrote into cleared buffers), each with its own sample count; `normal` may be NULL (the normal
 * test then always passes), `depth` is required.  `out` receives the MEAN (preview it with samples = 1, or hand it to
 * bt_denoise_device with color_samples = 1); out.a = the colour buffer's alpha.  Per pixel (x, y), in float32:
 *     c = C.rgb / n_c;  n = the normalised mean normal (0 if shorter than 1e-6);  z = D.r / n_d;  far = z >= 1
 *     first call since _new / _reset: out.rgb = c, history length = n_c
 *     `view` bitwise equal to the previous call's: the pixel's own history is taken, weight W = 1, untested (the same pose
 *     and a static world: a silhouette pixel whose samples hit in one frame and all miss in the next keeps its history)
 *     else the pixel's point -- the ray through the centre of its sample footprint at distance clip_min + z (clip_max -
 *     clip_min), or the ray's direction if far -- is projected into the previous view: (x_f, y_f) there, z' its
 *     normalised distance from the previous camera; the four bilinear taps of the previous history around (x_f, y_f): one is dropped if it lies outside the frame, if
 *     its depth z_q fails (far: z_q >= 1; else z_q < 1 and |z' - z_q| <= depth_tolerance z') or its normal n_q fails
 *     (both zero: pass; one zero: fail; else n . n_q >= normal_min); W = the surviving weight
 *     W < 1e-3: as on the first call; else m, h = the weighted history colour and length, N = min(h + n_c, max_history),
 *     a = min(1, max(n_c / N, alpha_min)), out.rgb = m + (c - m) a, history length = N.
 * A camera that does not move accumulates the running mean.  Depth-of-field origin jitter is ignored by the projection.
 * Checked before the device is touched, in this order, all BT_ERR_INVALID_ARG: NULL handle / view / colour / depth /
 * out; a sample count of 0 for a buffer that is given; view.width / height other than the handle's; a non-finite view
 * entry, a field of view <= 0, clip_max <= clip_min or a singular to_world (|det| < 1e-12); a parameter outside its
 * range; `out` equal to an input.  A valid call without a device returns BT_ERR_DEVICE.  params == NULL: the defaults.
 * Not provided: a variance history, moving objects, sharded frames, host buffers, the lens extension and adaptively
 * sampled frames (whose tiles hold different counts). */
int bt_temporal_accumulate_device(bt_temporal *t, const bt_view *view, const float *color, uint32_t color_samples,
                                  const float *normal, uint32_t normal_samples, const float *depth, uint32_t depth_samples,
                                  float *out, const bt_temporal_params *params, void *stream);
/* For tests: the current history plane, RGBA (rgb = accumulated mean, a = history length), row-major; zeros while there is
 * none.  n == 0 returns the number of floats, else up to n are copied to `host` (synchronises) and the number copied is
 * returned. */
int bt_debug_temporal_history(bt_temporal *t, float *host, uint32_t n);
/* For tests, on the host, by the code the kernel runs (bt_view.hpp): where pixel (x, y) of `cur` at normalised depth z
 * (z >= 1: at infinity) lies in `prev`: out = (x_f, y_f, z').  BT_ERR_INVALID_ARG for a view the accumulate would refuse. */
int bt_debug_reproject(const bt_view *cur, const bt_view *prev, float x, float y, float z, float *out);

/* --- EXTENSION -- NOT IN THE REFERENCE: display stage -- metered auto-exposure and tone mapping ----
 * Buffer::preview divides by the sample count, applies the sRGB curve and saturates at 1.0.  This stage is off unless
 * called, makes no parity claim and changes neither a render nor bt_preview*.  It meters the frame's luminance, derives an
 * exposure on the device, adapts it from frame to frame and maps the exposed mean through a tone operator into RGBA8.
 * The input is a frame of RGBA32F running sums with its sample count n (a mean is n = 1: what bt_denoise_device,
 * bt_temporal_accumulate_device and bt_adaptive_resolve_device write).  Everything is float32 in the order written, without
 * fused multiply-adds, with correctly rounded `/`:
 *   meter, per pixel:  r = 1 / n;  c = rgb * r;  Y = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z;
 *     !(Y >= 2^-16) -> `under` (zero, negatives, NaN);  else Y >= 2^16 -> `over` (+inf);  else bin (bits(Y) >> 20) - 888 of
 *     256: eight bins per octave (the exponent and three mantissa bits) over 32 octaves.  The counts h_b are uint32.
 *   expose, from the 256 counts (integers stay integers):  N = sum h_b;  lo = floor((double)p_low N);
 *     hi = N - floor((double)p_high N);  P_b = the exclusive prefix sum;  w_b = max(0, min(P_b + h_b, hi) - max(P_b, lo));
 *     W = sum w_b;  S = sum w_b (2 b + 1) (64-bit).  W == 0 (a black frame): the handle's state is left alone and the frame is
 *     shown with the state's exposure if there is one, else with params.ev.  Otherwise m = S / (16.0 W) - 16.0 in float64
 *     (the mean of the bin centres in log2), t = (float)(log2(key) - m) + ev with log2(key) formed once on the host in
 *     float64, t clamped to [ev_min, ev_max]; state (e, valid): e = t if !valid or adapt >= 1, else e = e + (t - e) adapt;
 *     valid = true.  mult = exp2(e) by the polynomial bt_preview's sRGB curve uses.
 *     auto_exposure == 0: neither meter nor expose runs, e = ev, mult = exp2(ev), the state is untouched.
 *   show, per pixel and channel:  x = c * mult;  BT_TONEMAP_CLIP: x;  the others first x = x > 0 ? x : 0, then
 *     BT_TONEMAP_REINHARD: x (1 + x iw2) / (1 + x) with iw2 = 1 / (white white) formed on the host;
 *     BT_TONEMAP_ACES (Narkowicz's fit): (x (2.51 x + 0.03)) / (x (2.43 x + 0.59) + 0.14);
 *     then the colour space (BT_COLOR_NONE / _LINEAR raw, _SRGB the sRGB curve) and the saturating conversion to 8 bits exactly
 *     as bt_preview_device has them; alpha = the buffer's alpha, converted the same way.  BT_TONEMAP_CLIP with
 *     auto_exposure == 0 and ev == 0 is bt_preview_device bit for bit. */
typedef enum { BT_TONEMAP_CLIP = 0, BT_TONEMAP_REINHARD = 1, BT_TONEMAP_ACES = 2 } bt_tonemap;
typedef struct {
    double key;                /* > 0, finite: the luminance the metered mean is brought to (a double: log2(key) is float64) */
    int32_t tonemap;           /* bt_tonemap */
    int32_t auto_exposure;     /* 0: show with `ev`; else meter the frame, `ev` is a compensation added to the metered exposure */
    float ev;                  /* finite; stops */
    float p_low, p_high;       /* [0, 1), p_low + p_high < 1: the darkest / brightest fraction of the pixels the meter ignores */
    float adapt;               /* (0, 1]: the fraction of the way to the new target one call moves; 1 = no memory */
    float ev_min, ev_max;      /* ev_min <= ev_max: the metered exposure is clamped to this range */
    float white;               /* > 0: BT_TONEMAP_REINHARD's white point, the exposed value that maps to 1 */
} bt_display_params;
typedef struct bt_display bt_display;     /* owns the counters and the adaptation state (2 KiB on the device); one stream at a time */
/* ACES, auto_exposure 1, ev 0, key 0.18, p_low 0.10, p_high 0.02, adapt 1, ev_min -8, ev_max +8, white 4. */
void bt_display_params_default(bt_display_params *out);
/* No device work happens here: the handle allocates on its first bt_display_device, on the device current then. */
bt_display *bt_display_new(void);
void bt_display_free(bt_display *d);
/* Forgets the adaptation state and the last call: the next metered frame sets the exposure outright. */
int bt_display_reset(bt_display *d);
/* Up to three kernels on `stream` (meter, expose, show; show alone with auto_exposure == 0); returns without synchronising,
 * the exposure never visits the host.  `rgba_device`: width * height RGBA32F running sums of `samples` samples;
 * `rgba8_device`: width * height RGBA8.  params == NULL: the defaults.  Checked before the device is touched, in this order,
 * all BT_ERR_INVALID_ARG: NULL handle, input or output; samples == 0; zero width or height (or 2^32 pixels and more); input
 * equal to output; a colour space other than BT_COLOR_NONE / _LINEAR / _SRGB (BT_COLOR_NORMAL is for the normal AOV); an
 * unknown operator; non-finite ev; key <= 0 or non-finite; p_low or p_high outside [0, 1) or p_low + p_high >= 1; adapt
 * outside (0, 1]; ev_min > ev_max (or either NaN); white <= 0 (or NaN).  A valid call without a device returns BT_ERR_DEVICE.
 * Not provided: a host-buffer variant, sharded frames, metering regions or weights, per-luminance (hue-preserving)
 * operators and dithering. */
int bt_display_device(bt_display *d, const float *rgba_device, uint32_t samples, uint8_t *rgba8_device, uint32_t width,
                      uint32_t height, int32_t color_space, const bt_display_params *params, void *stream);
/* The exposure the last bt_display_device showed its frame with, in stops, and its multiplier (synchronises).  Either
 * pointer may be NULL.  BT_ERR_INVALID_ARG while there is none: before the first call and after bt_display_reset. */
int bt_display_exposure(bt_display *d, float *ev, float *mult);
/* For tests: the counters of the last metered call -- 256 bins, then `under`, then `over` (258 in all); zeros while there is
 * none.  n == 0 returns 258, else up to n are copied to `host` (synchronises) and the number copied is returned. */
int bt_debug_display_histogram(bt_display *d, uint32_t *host, uint32_t n);
/* The linear frame as a Portable Float Map: "PF\n<width> <height>\n-1.0\n", then the rows bottom to top, per pixel
 * rgb * (1.0f / samples) as little-endian float32.  `rgba_host` is the frame of running sums on the host. */
int bt_write_pfm(const char *path, const float *rgba_host, uint32_t width, uint32_t height, uint32_t samples);

/* --- EXTENSION -- NOT IN THE REFERENCE: glare stage -- an energy-conserving bloom ahead of the display stage ----
 * The tone curve maps every emitter far above 1.0 to the same flat white.  Glare is light scattered in the eye or the lens: a
 * wide point-spread function applied in scene-linear light, before exposure and tone mapping.  This stage is off unless
 * called, makes no parity claim and changes neither a render nor bt_preview* nor bt_display_*.  The input is a frame of
 * RGBA32F running sums with its sample count n (a mean is n = 1); the output is a MEAN, as bt_denoise_device's is: preview or
 * display it with samples = 1.  Everything is float32 in the order written, without fused multiply-adds, with correctly
 * rounded `/` (csrc/bt_glare.hpp has the same lines as code; tests/glare_ref.py in numpy):
 *   1. sanitise, per pixel and channel:  r = 1 / n;  c = rgb * r;  s = c >= 0 ? c : 0 (NaN and negatives -> 0);
 *      s = s < max_value ? s : max_value (+inf and fireflies are capped).  The planes below carry rgb and a fourth channel of 0.
 *   2. L = min(levels, bit_length(max(width, height) - 1)); level k has sides ceil(side_{k-1} / 2);  D_0 = s.
 *   3. down, k = 1 .. L, separable, x then y.  Per axis, output i takes the taps a, b, c, d at 2i-1, 2i, 2i+1, 2i+2, each
 *      clamped to [0, side_{k-1} - 1]:  t = b + c;  D = (((a + d) + t) + (t + t)) * 0.125     (the binomial [1 3 3 1] / 8)
 *   4. weights, on the host in float64 by repeated multiplication:  p_1 = 1, p_k = p_{k-1} * (double)spread, S their sum in
 *      order, w_k = (float)(p_k / S).
 *   5. up:  A_L = D_L * w_L;  for k = L-1 .. 1:  A_k = D_k * w_k + up(A_{k+1}).  up is separable, x then y.  Per axis, output
 *      x takes near = x >> 1 and far = near - 1 (x even) or near + 1 (x odd), both clamped to the coarser side:
 *      ((far + near) + (near + near)) * 0.25                                                 (the tent [1 3] / 4)
 *   6. composite, per pixel:  G = up(A_1);  out.rgb = s + (G - s) * strength;  out.a = the input's a.
 *   7. L = 0 (levels = 0 or a 1 x 1 frame):  out.rgb = s.
 * The filter is linear and non-negative and each level's weights sum to 1 away from the border, so an impulse keeps its
 * energy.  There is no brightness threshold and no dependence on exposure: the stage commutes with the exposure multiplier. */
typedef struct {
    uint32_t levels;           /* <= 16; the effective number is limited by the frame (step 2) */
    float spread;              /* (0, 16], finite: each coarser level weighs `spread` times the one before */
    float strength;            /* [0, 1]: the fraction of the light that is scattered */
    float max_value;           /* > 0, finite: the cap of step 1 */
} bt_glare_params;
typedef struct bt_glare bt_glare;         /* owns the pyramid: float4 planes, < 5.4 B per pixel (A_k overwrites D_k); one stream at a time */
/* levels 6, spread 1, strength 0.08, max_value 65536 (the display meter's `over` boundary).  Starting values, not tuned. */
void bt_glare_params_default(bt_glare_params *out);
/* No device work happens here: the handle allocates on its first bt_glare_device, on the device current then, and grows on
 * demand. */
bt_glare *bt_glare_new(void);
void bt_glare_free(bt_glare *g);
/* 2 L kernels on `stream` (one for L = 0); returns without synchronising.  `rgba_device`: width * height RGBA32F running sums of
 * `samples` samples; `out_device`: width * height RGBA32F, the glared mean.  params == NULL: the defaults.  Checked before
 * the device is touched, in this order, all BT_ERR_INVALID_ARG: NULL handle, input or output; samples == 0; zero width or
 * height (or 2^32 pixels and more); output equal to input; levels > 16; spread not finite or outside (0, 16]; strength outside
 * [0, 1] (or NaN); max_value not finite or <= 0.  A valid call without a device returns BT_ERR_DEVICE, and so does a frame
 * whose 16 x 16 tiles do not fit one launch (2^24 tiles and more).
 * Not provided: host buffers, sharded frames, anisotropic or spectral point-spread functions, a brightness threshold. */
int bt_glare_device(bt_glare *g, const float *rgba_device, uint32_t samples, float *out_device, uint32_t width, uint32_t height,
                    const bt_glare_params *params, void *stream);
/* For tests: plane A_k (k = 1 .. L of the last call) as RGBA float, the fourth channel 0.  n == 0 returns the element count,
 * else up to n floats are copied to `host` (synchronises) and the number copied is returned.  BT_ERR_INVALID_ARG for a
 * level the last call did not have. */
int bt_debug_glare_plane(bt_glare *g, uint32_t level, float *host, uint32_t n);
/* For tests, no device: the whole definition on the host through csrc/bt_glare.hpp's own functions.  The same checks as
 * bt_glare_device without the handle. */
int bt_debug_glare_host(const float *rgba_host, uint32_t samples, float *out_host, uint32_t width, uint32_t height,
                        const bt_glare_params *params);

/* --- EXTENSION -- NOT IN THE REFERENCE: resample stage -- render at one size, show at another -------------------
 * A separable filter from a frame of w x h RGBA32F running sums with its sample count n (a mean is n = 1) to a MEAN of W x H, any
 * W, H >= 1, each axis larger, smaller or equal on its own.  It sits after the glare stage and before the display stage, in
 * scene-linear light, so exposure is metered on what is shown.  The reference's viewer resizes its buffer to the window
 * (main.rs:338-342) and has no such filter: this stage is off unless called, makes no parity claim and changes neither a render
 * nor bt_preview*, bt_display_*, bt_glare_*, bt_denoise* or bt_temporal_*.  Pixels are float32 in the order written, without
 * fused multiply-adds; the weight tables are float64 on the host (csrc/bt_resample.hpp has the same lines as code;
 * tests/resample_ref.py in numpy):
 *   1. sanitise: the glare stage's step 1, the same function -- r = 1 / n; c = rgb * r; NaN and negatives -> 0; capped at
 *      max_value.  It precedes every tap: a NaN does not spread over a filter footprint.
 *   2. tables, per axis (src -> dst texels), built once per (src, dst, filter) and kept on the handle:  ratio = (double)src / dst;
 *      s = max(1, ratio);  c_i = (i + 0.5) * ratio - 0.5;  taps j = ceil(c_i - R s) .. floor(c_i + R s) with R = 0.5, 1, 2, 3 for
 *      box, tent, mitchell, lanczos3;  k_j = k((j - c_i) / s);  S = their sum in ascending j;  w_ij = (float)(k_j / S).  T is the
 *      axis's largest tap count; shorter rows are padded with weights 0.  nearest_i = min(src - 1, floor((i + 0.5) * ratio)).
 *      k: box 1 on [-0.5, 0.5); tent 1 - |x|; mitchell the B = C = 1/3 cubic as (((21a - 36)a)a + 16) / 18 for a = |x| < 1 and
 *      (((-7a + 36)a - 60)a + 32) / 18 for 1 <= a < 2; lanczos3 (sin(p) / p) * (sin(q) / q) with p = pi x, q = p / 3, exactly 1 at
 *      0 and exactly 0 at every other x == rint(x); every k is 0 outside its support.
 *   3. horizontal: P(i, y) = sum over the T_x taps of w * s(clamp(j, 0, w - 1), y), as acc = 0; acc = acc + w * v in ascending j,
 *      the product rounded, then the sum; a tap clamped to the border keeps its own weight (edge replication).  P is W x h.
 *   4. vertical: the same over P with the y table -> W x H.
 *   5. clamp_negative: out = acc >= 0 ? acc : 0 (mitchell and lanczos3 have negative lobes and undershoot next to an emitter).
 *   6. out.a = the input's a at (nearest_x, nearest_y): not filtered, not divided by n.
 * At W x H = w x h tent and lanczos3 return the sanitised mean bit for bit; box at w = 2 W has the weights 0.5, 0.5. */
typedef enum { BT_RESAMPLE_BOX = 0, BT_RESAMPLE_TENT = 1, BT_RESAMPLE_MITCHELL = 2, BT_RESAMPLE_LANCZOS3 = 3 } bt_resample_filter;
typedef struct {
    int32_t filter;            /* a bt_resample_filter */
    float max_value;           /* > 0, finite: the cap of step 1 */
    int32_t clamp_negative;    /* step 5: 0 keeps the undershoot */
} bt_resample_params;
typedef struct bt_resample bt_resample;   /* owns P (16 B per texel of W x h) and both tables, host and device; one stream at a time */
/* mitchell, max_value 65536 (the glare stage's cap), clamp_negative 1. */
void bt_resample_params_default(bt_resample_params *out);
/* No device work happens here: the handle allocates on its first bt_resample_device, on the device current then, and grows on
 * demand. */
bt_resample *bt_resample_new(void);
void bt_resample_free(bt_resample *h);
/* Two kernels on `stream`, one per pass, after the uploads of a table that changed (on `stream` too); returns without
 * synchronising, except that a call which replaces a table first waits for the handle's previous call, whose upload may still
 * read it.  `rgba_device`: width * height RGBA32F running sums of `samples` samples; `out_device`: out_width * out_height
 * RGBA32F, the mean.  params == NULL: the defaults.  Checked before the device is touched, in this order, all
 * BT_ERR_INVALID_ARG: NULL handle, input or output; samples == 0; a zero side, a side of 2^31 and more or 2^32 pixels and more,
 * on either frame; output equal to input; a filter that is no bt_resample_filter; max_value not finite or <= 0; T > 128 on the
 * x axis, then on the y axis (lanczos3 beyond about 21 : 1, mitchell 32 : 1, tent 64 : 1, box 127 : 1; the message names the axis
 * and the ratio).  A valid call without a device returns BT_ERR_DEVICE, and so does a plane whose 32 x 8 tiles do not fit one
 * launch (2^24 tiles and more).
 * Not provided: host buffers, sharded frames, resampling of the albedo / normal / depth
 * outputs (step 1 would clamp them), any change to the size the render kernels work at.  Guide-driven upsampling is bt_upscale's. */
int bt_resample_device(bt_resample *h, const float *rgba_device, uint32_t samples, uint32_t width, uint32_t height, float *out_device,
                       uint32_t out_width, uint32_t out_height, const bt_resample_params *params, void *stream);
/* For tests: the table of axis 0 (x) or 1 (y) that the handle's last call -- bt_resample_device or bt_debug_resample_host --
 * built or reused.  Returns T.  Any pointer may be NULL; `sides` receives {src, dst, filter}, `first` the dst first taps
 * (unclamped: first_i + t is clamped where it is used), `weights` dst rows of T, `nearest` the dst nearest source indices.
 * BT_ERR_INVALID_ARG while there is no table. */
int bt_debug_resample_weights(bt_resample *h, int axis, uint32_t *sides, int32_t *first, float *weights, uint32_t *nearest);
/* For tests: P of the last bt_resample_device as RGBA float, out_width x height, the fourth channel 0.  n == 0 returns the element
 * count, else up to n floats are copied to `host` (synchronises) and the number copied is returned. */
int bt_debug_resample_plane(bt_resample *h, float *host, uint32_t n);
/* For tests, no device: the whole definition on the host through csrc/bt_resample.hpp's own functions.  The same checks as
 * bt_resample_device; `h` may be NULL, else the tables are the handle's (kept for bt_debug_resample_weights). */
int bt_debug_resample_host(bt_resample *h, const float *rgba_host, uint32_t samples, uint32_t width, uint32_t height, float *out_host,
                           uint32_t out_width, uint32_t out_height, const bt_resample_params *params);

/* --- EXTENSION -- NOT IN THE REFERENCE: despeckle stage -- rank-order firefly rejection ahead of the chain -------
 * A path tracer at low sample counts leaves single pixels far brighter than anything around them, and every later stage makes
 * them worse: the denoiser's colour stop keeps them as edges, the temporal history takes many frames to forget them, the glare
 * stage turns each into a halo and a filter with negative lobes rings around it.  This stage pulls a pixel whose luminance
 * exceeds `ratio` times the `rank`-th brightest of its neighbours down to that limit.  It is off unless called, makes no parity
 * claim and changes neither a render nor any other stage.  The input is a frame of RGBA32F running sums with its sample count n
 * (a mean is n = 1); the output is in the input's units -- SUMS of the same n, not a mean -- so the stage can stand in front of
 * bt_temporal_accumulate_device without falsifying its history lengths, and anywhere else in the chain.  Everything is float32
 * in the order written, without fused multiply-adds, with correctly rounded `/` (csrc/bt_despeckle.hpp has the same lines as
 * code; tests/despeckle_ref.py in numpy):
 *   1. on the host:  fn = (float)n;  cap = max_value * fn;  fl = floor * fn.
 *   2. sanitise, per pixel and channel of rgb:  s = v >= 0 ? v : 0 (NaN and negatives -> 0);  s = s < cap ? s : cap;
 *      Y = (0.2126 * s.x + 0.7152 * s.y) + 0.0722 * s.z, the display meter's luminance.
 *   3. the neighbours of pixel (x, y) are the in-frame pixels of the (2 radius + 1)^2 window, centre excluded.  Out-of-frame taps
 *      are absent, not clamped (with replicated borders a corner pixel would be three of its own eight neighbours and could
 *      never be flagged):  M = (min(x + R, W - 1) - max(x - R, 0) + 1) * (min(y + R, H - 1) - max(y - R, 0) + 1) - 1;
 *      k = min(rank, M);  a pixel with M = 0 is never flagged.
 *   4. T = the k-th largest neighbour Y (1 = the brightest): an order statistic of non-negative finite floats, whose value does
 *      not depend on how it is selected.
 *   5. lim = T * ratio + fl.
 *   6. Y > lim: the pixel is flagged, g = lim / Y, out.rgb = s * g.  Otherwise out.rgb = s.  In both cases out.a = the input's a.
 * Every neighbour value is the input's: the stage is single pass and order-free.  A clean, unflagged pixel comes back bit for
 * bit, -0.0 included.  A bright feature survives where every pixel of it has at least `rank` neighbours as bright as itself,
 * within `ratio`: at radius 1, rank 2 isolated pixels and adjacent pairs are pulled down, 2 x 2 blocks, L-shaped triples and the
 * interior of a one-pixel line are kept -- and the two end pixels of such a line are not. */
typedef struct {
    uint32_t radius;           /* 1 or 2: the window is (2 radius + 1)^2 */
    uint32_t rank;             /* 1 .. (2 radius + 1)^2 - 1 */
    float ratio;               /* >= 1, finite */
    float floor;               /* >= 0, finite: in units of the mean, so that a pixel in a black neighbourhood is judged against it */
    float max_value;           /* > 0, finite: the cap of step 2, in units of the mean */
} bt_despeckle_params;
typedef struct {
    uint32_t flagged;          /* pixels step 6 pulled down */
    uint32_t sanitised;        /* pixels in which step 2 changed a channel */
    uint32_t pixels;           /* width * height of the call */
    uint32_t reserved;
} bt_despeckle_stats;
typedef struct bt_despeckle bt_despeckle;   /* owns two uint32 counters on the device; one stream at a time */
/* radius 1, rank 2, ratio 4, floor 0.01, max_value 65536 (the glare stage's cap).  Starting values; DESIGN.md 18 has the sweep. */
void bt_despeckle_params_default(bt_despeckle_params *out);
/* No device work happens here: the handle allocates its counters on its first bt_despeckle_device, on the device current then. */
bt_despeckle *bt_despeckle_new(void);
void bt_despeckle_free(bt_despeckle *h);
/* One kernel on `stream`, after the counters have been zeroed on it; returns without synchronising.  `rgba_device`: width *
 * height RGBA32F running sums of `samples` samples; `out_device`: width * height RGBA32F, sums of the same count.  params ==
 * NULL: the defaults.  Checked before the device is touched, in this order, all BT_ERR_INVALID_ARG: NULL handle, input or
 * output; samples == 0; zero width or height (or 2^32 pixels and more); output equal to input; radius other than 1 or 2;
 * rank == 0 or rank > (2 radius + 1)^2 - 1; ratio not finite or < 1; floor not finite or < 0; max_value not finite or <= 0.  A
 * valid call without a device returns BT_ERR_DEVICE, and so does a frame whose 16 x 16 tiles do not fit one launch (2^24 tiles
 * and more).
 * Not provided: host buffers, sharded frames (a shard is tile-major and the window crosses tiles), per-sample clamping inside
 * the render kernel, the guides or the adaptive moment plane as the statistic. */
int bt_despeckle_device(bt_despeckle *h, const float *rgba_device, uint32_t samples, float *out_device, uint32_t width, uint32_t height,
                        const bt_despeckle_params *params, void *stream);
/* The counts of the last bt_despeckle_device (synchronises its stream).  Both are integers, so they are deterministic.
 * BT_ERR_INVALID_ARG before any call. */
int bt_despeckle_poll(bt_despeckle *h, bt_despeckle_stats *out);
/* For tests, no device and no handle: the whole definition on the host through csrc/bt_despeckle.hpp's own functions,
 * single-threaded.  The same checks as bt_despeckle_device without the handle.  `stats` may be NULL. */
int bt_debug_despeckle_host(const float *rgba_host, uint32_t samples, float *out_host, uint32_t width, uint32_t height,
                            const bt_despeckle_params *params, bt_despeckle_stats *stats);

/* --- EXTENSION -- NOT IN THE REFERENCE: upscale stage -- guide-driven upsampling of a small render --------------
 * Joint bilateral upsampling (Kopf et al., SIGGRAPH 2007): lighting is rendered at w x h, the albedo, normal and depth guides
 * (the BT_OUTPUT_ALBEDO / _NORMAL / _DEPTH frames, as bt_denoise* takes them) at w x h AND at the shown size W x H, where a
 * guide-only render ends at the first hit.  A lo texel contributes to an output pixel by its bilinear weight times how well its
 * guides match the pixel's own, so a light's radiance is not smeared over the wall next to it.  The stage sits after the
 * denoiser and before the glare stage, whose halos legitimately cross edges.  It is off unless called, makes no parity claim
 * and changes neither a render nor any other stage.  The output is a MEAN of W x H, W >= w and H >= h, each axis on its own,
 * equality allowed.  Pixels are float32 in the order written, without fused multiply-adds; only + - * / and sqrt appear, all
 * correctly rounded (no exp, no pow); the per-axis tables are float64 on the host (csrc/bt_upscale.hpp has the same lines as
 * code; tests/upscale_ref.py in numpy):
 *   1. prepare, at either size, r = 1 / n once per frame:  colour c = the glare stage's step 1 (NaN and negatives -> 0, capped at
 *      max_value);  fin(v) = |v| < inf ? v : 0;  albedo a = fin(A.rgb * r_a);  normal v = fin(N.rgb * r_n), l = (v.x v.x + v.y v.y) +
 *      v.z v.z, n = l > 1e-12 ? v / sqrt(l) : 0 -- a zero normal marks a miss;  depth z = fin(Z.r * r_z).  An absent pair is all
 *      zeros on both sides, which weighs exactly 1.
 *   2. tables, per axis (src -> dst texels), built once per (src, dst) and kept on the handle:  ratio = (double)src / dst;
 *      c_i = (i + 0.5) * ratio - 0.5;  x0 = floor(c_i);  f = c_i - x0;  the four taps are x0 - 1 + t, t = 0 .. 3, d_t = t - 1, each
 *      clamped to [0, src - 1] where it is used, keeping its weight (edge replication);  u1_t = (float)max(0, 1 - |d_t - f|);
 *      u2_t = (float)max(0, 1 - |d_t - f| * 0.5);  nearest_i = min(src - 1, floor((i + 0.5) * ratio)).
 *   3. per output pixel p, its 16 taps q, ty outer and tx inner:
 *        g_n = 1 if both normals are zero, 0 if exactly one is, else m = max((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z, 0) squared
 *              normal_squarings times;
 *        g_z = 1 / (1 + t * t),  t = |z_p - z_q| / (sigma_depth * z_p + 1e-6);
 *        g_a = 1 / (1 + s * k_a),  d = a_p - a_q,  s = (d.x d.x + d.y d.y) + d.z d.z,  k_a = 1 / (sigma_albedo * sigma_albedo) in
 *              float32 on the host;
 *        g = (g_n * g_z) * g_a;  s1 = u1y * u1x;  s2 = u2y * u2x;  w1 = s1 * g;  w2 = s2 * g;
 *        A1 += w1 * c_q, D1 += w1;  A2 += w2 * c_q, D2 += w2;  A0 += s1 * c_q, D0 += s1 -- each as acc = acc + w * c per channel,
 *        the product rounded, then the sum, over all 16 taps, those of weight 0 too.
 *   4. out.rgb = A1 / D1 where D1 > min_weight (tier 1: the 2 x 2 bilinear footprint with guides), else A2 / D2 where D2 >
 *      min_weight (tier 2: the 4 x 4 footprint, for a pixel whose four nearest texels all lie across an edge), else A0 / D0
 *      (tier 3: plain bilinear).  out.a = C.a at (nearest_x, nearest_y), neither filtered nor divided by n.
 *   5. the handle counts the pixels of the last call that took tier 2 and tier 3.
 * With no pair at all the stage is a bilinear resize.  At W x H = w x h, with the same frames as lo and hi guides and no normal
 * pair, the output is the sanitised mean bit for bit and both counts are 0 (with the normal pair n . n can be 1 - ulp). */
typedef struct {
    float sigma_depth;         /* > 0, finite: the relative depth difference at which g_z is 1/2 */
    float sigma_albedo;        /* > 0, finite: the albedo distance at which g_a is 1/2 */
    uint32_t normal_squarings; /* 0 .. 6: g_n = max(n_p . n_q, 0)^(2^normal_squarings) */
    float min_weight;          /* in (0, 1), finite: the D below which a tier is given up */
    float max_value;           /* > 0, finite: the cap of step 1 */
} bt_upscale_params;
/* One frame's guides: running sums of RGBA32F with their sample counts (a mean is 1); NULL marks an absent guide. */
typedef struct {
    const float *albedo;
    uint32_t albedo_samples;
    const float *normal;
    uint32_t normal_samples;
    const float *depth;
    uint32_t depth_samples;
} bt_upscale_guides;
typedef struct {
    uint32_t tier2;            /* output pixels that took the 4 x 4 footprint */
    uint32_t tier3;            /* output pixels that fell back to plain bilinear */
    uint32_t pixels;           /* out_width * out_height of the call */
    uint32_t reserved;
} bt_upscale_stats;
typedef struct bt_upscale bt_upscale;   /* owns the three prepared planes (48 B per texel of w x h), both tables and a counter; one stream at a time */
/* sigma_depth 0.1, sigma_albedo 0.1, normal_squarings 3 (the 8th power), min_weight 0.01, max_value 65536 (the glare stage's cap).
 * Starting values; DESIGN.md 19 has the sweep. */
void bt_upscale_params_default(bt_upscale_params *out);
/* No device work happens here: the handle allocates on its first bt_upscale_device, on the device current then, and grows on
 * demand. */
bt_upscale *bt_upscale_new(void);
void bt_upscale_free(bt_upscale *h);
/* Two kernels on `stream` (prepare, upscale), after the counter has been zeroed and a table that changed has been uploaded on
 * it; returns without synchronising, except that a call which replaces a table first waits for the handle's previous call, whose
 * upload may still read it.  `color_device`: width * height RGBA32F running sums of `color_samples` samples; `lo`: the guides at
 * width x height, `hi`: at out_width x out_height, either NULL for none; `out_device`: out_width * out_height RGBA32F, the mean.
 * params == NULL: the defaults.  Checked before the device is touched, in this order, all BT_ERR_INVALID_ARG: NULL handle, colour
 * or output; color_samples == 0; a zero side, a side of 2^31 and more or 2^32 pixels and more, on either frame; out_width <
 * width or out_height < height (bt_resample reduces); output equal to the colour frame or to any guide; a guide present at
 * one size only; a present guide with 0 samples; sigma_depth, sigma_albedo not finite or <= 0; normal_squarings > 6; min_weight
 * outside (0, 1); max_value not finite or <= 0.  A valid call without a device returns BT_ERR_DEVICE, and so does a frame whose
 * 16 x 16 tiles do not fit one launch (2^24 tiles and more).
 * Not provided: host buffers, sharded frames, downscaling, any change to bt_resample or bt_denoise. */
int bt_upscale_device(bt_upscale *h, const float *color_device, uint32_t color_samples, uint32_t width, uint32_t height,
                      const bt_upscale_guides *lo, const bt_upscale_guides *hi, float *out_device, uint32_t out_width, uint32_t out_height,
                      const bt_upscale_params *params, void *stream);
/* The counts of the last bt_upscale_device (synchronises its stream).  They are integers, so they are deterministic.
 * BT_ERR_INVALID_ARG before any call. */
int bt_upscale_poll(bt_upscale *h, bt_upscale_stats *out);
/* For tests: the table of axis 0 (x) or 1 (y) that the handle's last call -- bt_upscale_device or bt_debug_upscale_host with a
 * handle -- built or reused.  Returns 8, the weights per row.  Any pointer may be NULL; `sides` receives {src, dst}, `first` the dst
 * first taps x0 - 1 (unclamped), `weights` dst rows of u1_0 .. u1_3, u2_0 .. u2_3, `nearest` the dst nearest source indices.
 * BT_ERR_INVALID_ARG while there is no table. */
int bt_debug_upscale_weights(bt_upscale *h, int axis, uint32_t *sides, int32_t *first, float *weights, uint32_t *nearest);
/* For tests: a prepared lo plane of the last bt_upscale_device as width x height float4 -- which = 0: (c.rgb, z), 1: (n.xyz, 0),
 * 2: (a.rgb, 0).  n == 0 returns the element count, else up to n floats are copied to `host` (synchronises) and the number copied
 * is returned. */
int bt_debug_upscale_plane(bt_upscale *h, uint32_t which, float *host, uint32_t n);
/* For tests, no device: the whole definition on the host through csrc/bt_upscale.hpp's own functions, single-threaded.  The
 * same checks as bt_upscale_device; `h` may be NULL, else the tables are the handle's (kept for bt_debug_upscale_weights).
 * `stats` may be NULL. */
int bt_debug_upscale_host(bt_upscale *h, const float *color_host, uint32_t color_samples, uint32_t width, uint32_t height,
                          const bt_upscale_guides *lo, const bt_upscale_guides *hi, float *out_host, uint32_t out_width, uint32_t out_height,
                          const bt_upscale_params *params, bt_upscale_stats *stats);

/* --- EXTENSION -- NOT IN THE REFERENCE: compare stage -- deterministic image-error metrics on the device --------
 * How far a test frame X is from a reference frame Y: MSE, relMSE, PSNR, SSIM, the largest difference, the share of the error
 * that the worst pixels carry, and a false-colour error map.  It measures the chain and is no part of it: nothing here changes a
 * frame.  Both frames are width * height RGBA32F running sums on the device with their sample counts (a mean has count 1); alpha
 * is ignored; the two may be the same pointer.  Everything is float64 unless marked float32, computed in the order written
 * (-ffp-contract=off) with + - * /, max and compares only, so the device, the host entry point and numpy agree bit for bit
 * (csrc/bt_compare.hpp has the same lines as code; tests/compare_ref.py in numpy):
 *   1. point      float32: r = 1 / n; x = X.rgb * r_x, y = Y.rgb * r_y.  A pixel is BAD if any of the six fails |v| < inf: it
 *                 counts in `nonfinite`, is not in `valid`, and all its terms are 0.  Else, in float64, per channel d = x - y,
 *                 e = d d, q = e / (y y + epsilon); se = (e.r + e.g) + e.b; re = (q.r + q.g) + q.b; m = max |d|.  The error
 *                 plane, float32: E = re < FLT_MAX ? (float)re : FLT_MAX; a bad pixel holds -0.0f (== 0, sign bit set).
 *   2. structure  float32: Yf = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z on x and on y; Yc = Yf > 0 ? min(Yf, FLT_MAX) : 0; a bad
 *                 pixel holds 0 on both sides.  float64: v = Yc / (1 + Yc).
 *   3. SSIM       11 taps of sigma 1.5 (literal weights); vx, vy, vx vx, vy vy, vx vy are blurred along x, then along y, with
 *                 edge replication, acc = acc + W[k] a[clamp(i + k - 5)] from acc = 0; sx = xx - mx mx, sy = yy - my my, cxy =
 *                 xy - mx my; s = ((2 (mx my) + C1)(2 cxy + C2)) / (((mx mx + my my) + C1)((sx + sy) + C2)), C1 = 1e-4, C2 = 9e-4.
 *   4. sums       per 16 x 16 tile a fixed tree over the 256 slots (stride 128, 64 .. 1), 0.0 outside the frame; the tiles'
 *                 partials are added one after another in tile order on the host.  No float atomic anywhere.
 *   5. results    below.  psnr = 10 log10(peak peak / mse) is formed on the host and is the one field that depends on a math
 *                 library; +inf for mse == 0.
 * One handle serves one stream at a time. */
typedef struct bt_compare_params {
    double epsilon;         /* relMSE's denominator offset; finite and > 0 */
    double peak;            /* PSNR's peak value; finite and > 0 */
} bt_compare_params;
typedef struct bt_compare_stats {
    uint64_t pixels, valid, nonfinite;
    uint64_t max_index;     /* the smallest y * width + x that attains max_abs */
    double mse;             /* S_se / (3 valid); 0 without a valid pixel */
    double rel_mse;         /* S_re / (3 valid); 0 without a valid pixel */
    double ssim;            /* S_s / pixels */
    double max_abs;
    double psnr;
} bt_compare_stats;
typedef struct bt_compare bt_compare;   /* owns the planes E, (vx, vy) and s (28 B per pixel), a slab of one slot per tile and the histograms */

/* epsilon 0.01, peak 1.0. */
void bt_compare_params_default(bt_compare_params *out);
/* No device work happens here: the handle allocates on its first bt_compare_device, on the device current then, and grows on
 * demand, never per call. */
bt_compare *bt_compare_new(void);
void bt_compare_free(bt_compare *h);
/* Two kernels on `stream` (point, SSIM); returns without synchronising.  Checked before the device is touched, in this order, all
 * BT_ERR_INVALID_ARG: NULL handle, frame or params; a sample count of 0; a zero side, a side of 2^31 and more or 2^32 pixels and
 * more; epsilon, then peak, not finite or <= 0.  A valid call without a device returns BT_ERR_DEVICE, and so does a frame whose
 * 16 x 16 tiles do not fit one launch (2^24 tiles and more). */
int bt_compare_device(bt_compare *h, const float *test_device, uint32_t test_samples, const float *ref_device, uint32_t ref_samples,
                      uint32_t width, uint32_t height, const bt_compare_params *params, void *stream);
/* The results of the last bt_compare_device (synchronises its stream; the frame sums are formed here, in tile order).
 * BT_ERR_INVALID_ARG before any call. */
int bt_compare_poll(bt_compare *h, bt_compare_stats *out);
/* The share of S_all = sum E that the worst `fraction` of the valid pixels of the last call carry (synchronises):
 * k = clamp(ceil(fraction valid), 1, valid); T = the k-th largest E, found exactly by a radix select over the float32 bit patterns
 * (three passes of 11, 11 and 10 bits, a 2 048-bin integer histogram each); c_gt = #(E > T), S_gt = the sum of (double)E over
 * those; share = (S_gt + (k - c_gt) (double)T) / S_all, 0 when S_all == 0.  `threshold` receives T.  Either pointer may be NULL.
 * BT_ERR_INVALID_ARG for a fraction outside (0, 1] and before any call. */
int bt_compare_tail(bt_compare *h, double fraction, double *share, float *threshold);
/* The error plane of the last call as RGBA8 on `stream` (one kernel; does not synchronise): in float32 t = min(E / scale, 1),
 * r = min(3 t, 1), g = clamp(3 t - 1, 0, 1), b = clamp(3 t - 2, 0, 1), each stored as (uint8)(v 255 + 0.5), alpha 255; a bad
 * pixel is (255, 0, 255).  BT_ERR_INVALID_ARG for a NULL pointer, a scale that is not finite or not > 0, and before any call. */
int bt_compare_map_device(bt_compare *h, uint8_t *rgba8_device, float scale, void *stream);
/* For tests: a plane of the last bt_compare_device -- which = 0: E, float32; 1: (vx, vy), float64 pairs; 2: s, float64.  n == 0
 * returns the element count (two per pixel for plane 1), else up to n elements are copied to `host` (synchronises) and the number
 * copied is returned. */
int bt_debug_compare_plane(bt_compare *h, uint32_t which, void *host, uint32_t n);
/* For tests, no device: the whole definition on the host through csrc/bt_compare.hpp's own functions, single-threaded.  The same
 * checks as bt_compare_device.  `stats` and the planes (width * height floats, pairs of doubles, doubles) may be NULL; with
 * n_tail > 0 the tail of each of `fractions` is written to `shares` and `thresholds`. */
int bt_debug_compare_host(const float *test_host, uint32_t test_samples, const float *ref_host, uint32_t ref_samples, uint32_t width,
                          uint32_t height, const bt_compare_params *params, bt_compare_stats *stats, float *e_host, double *v_host,
                          double *s_host, uint32_t n_tail, const double *fractions, double *shares, float *thresholds);
/* Reads a Portable Float Map: "PF" (colour) or "Pf" (grey, replicated to three channels), either byte order by the sign of the
 * scale, whose magnitude is ignored.  `rgba_host` receives the rows top-down (undoing bt_write_pfm's flip) as RGBA with alpha 1;
 * with rgba_host == NULL only *width and *height are written.  A missing file -> BT_ERR_IO; a malformed or truncated one ->
 * BT_ERR_PARSE; capacity_floats < 4 width height -> BT_ERR_INVALID_ARG. */
int bt_read_pfm(const char *path, float *rgba_host, size_t capacity_floats, uint32_t *width, uint32_t *height);

/* --- EXTENSION -- NOT IN THE REFERENCE: ray queries -- closest hits for the caller's rays, picking, autofocus ---
 * "What does this ray hit?", answered by the intersection code the render kernels run: `try_hit` (tracer/mod.rs:389-402) for ray i
 * with the clip [tmin, tmax] taken from the ray.  Off unless called; changes no render and no stage.
 *   - objects are visited in ascending ObjectRef and every accepted hit shrinks clip.max; a sphere or a plain rect accepts
 *     t <= clip.max, a cuboid face only t < clip.max (cuboid.rs:96): among exact ties the later plain object wins, the earlier of
 *     two cuboids wins, and a rect beats a coplanar cuboid face in either order;
 *   - `dir` is used as given and never normalised (the sphere quadratic assumes unit length: the caller's business, as it is
 *     Ray::new's in the reference); position = origin + dir * t;
 *   - sphere: normal = (position - centre) / radius, flipped and BT_FACE_BACK where dot(dir, normal) >= 0; a sphere that carries a
 *     volume reports the VOLUME_ faces.  Rect: rect.rs:138-142 (p < 0 is the front).  Nothing marches: volumes are surfaces here;
 *   - material_ref / volume_ref are the DataRefs of the row that was hit (a cuboid's faces carry their own materials), volume_ref
 *     UINT64_MAX where there is none; `prim` is the row of bt_scene_export_prims, so a cuboid's face is identifiable;
 *   - a miss: t = +inf, face = prim = -1, the three refs UINT64_MAX, position and normal 0.  A ray misses if any of its floats
 *     other than tmax is not finite, if tmax is NaN, or if tmin > tmax; tmax = +inf is allowed. */
typedef struct { float origin[3]; float tmin; float dir[3]; float tmax; } bt_ray;      /* 32 B */
/* ray.rs:9-15 in the oracle's numbering; 2 (Face::Volume) exists only inside a march and never appears here */
enum { BT_FACE_MISS = -1, BT_FACE_FRONT = 0, BT_FACE_BACK = 1, BT_FACE_VOLUME_FRONT = 3, BT_FACE_VOLUME_BACK = 4 };
typedef struct {
    float position[3]; float t;
    float normal[3];   int32_t face;
    uint64_t object_ref, material_ref;
    uint64_t volume_ref; int32_t prim; uint32_t reserved;
} bt_hit;                                                                              /* 64 B */
/* One kernel on `stream`: hits_device[i] answers rays_device[i], i < n.  Returns the number of rays enqueued and does not
 * synchronise.  Checked before the device is touched, in this order: NULL scene, rays or hits -> BT_ERR_INVALID_ARG; a pointer
 * that is not 16-byte aligned, or rays == hits -> BT_ERR_INVALID_ARG; n >= 2^30 -> BT_ERR_INVALID_ARG; a lens set on the scene ->
 * BT_ERR_UNSUPPORTED (queries are straight rays); n == 0 -> 0, nothing is launched.  A valid call without a device returns
 * BT_ERR_DEVICE.  The scene's tables are flattened and uploaded if they are stale; no render state of the handle changes. */
int bt_query_rays_device(bt_scene *scene, const bt_ray *rays_device, uint32_t n, bt_hit *hits_device, void *stream);
/* One kernel on `stream`, no scene: the rays through the footprint centres (bt_view above; csrc/bt_view.hpp `forward`) of the
 * pixels x0 <= x < x0 + w, y0 <= y < y0 + h, row-major, into rays_device[w * h]: origin = the view's translation, tmin = clip_min,
 * tmax = clip_max.  Checked before the device is touched, all BT_ERR_INVALID_ARG: NULL view or rays, or rays not 16-byte aligned;
 * a view the temporal stage refuses; an empty rectangle; a rectangle that leaves the frame.  Returns the number of rays. */
int bt_view_rays_device(const bt_view *view, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, bt_ray *rays_device, void *stream);
/* Synchronous convenience: bt_scene_camera_view, one view ray through pixel (x, y), one query, and the copy back.  Returns 1 for
 * a hit, 0 for a miss, < 0 on error (the two calls' own, and BT_ERR_INVALID_ARG for a NULL hit or a pixel outside the frame).
 * `focus` may be NULL; on a hit it receives the camera focus that puts the hit point in the focal plane, t * |d_cam.z| with d_cam
 * the pixel's camera-space direction: the inverse of the render kernel's `dw * (focus / |d_cam.z|)` (mod.rs:286-299), so it
 * holds under a scaled camera matrix too. */
int bt_scene_pick(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render, uint32_t width,
                  uint32_t height, uint32_t x, uint32_t y, bt_hit *hit, float *focus);
/* Replaces the camera's focus IN PLACE, as bt_scene_set_camera_pose replaces its pose: has_focus == 0 clears it (`focus: null`,
 * no depth of field).  The saved JSON is not updated.  The cached block masks are keyed by the focus and do not survive the
 * change.  BT_ERR_INVALID_REF / BT_ERR_NOT_CAMERA as the pose setter; with has_focus set, a focus that is not finite or is <= 0
 * -> BT_ERR_INVALID_ARG.
 * Not provided: an any-hit or occlusion variant, host-buffer variants, the lens extension, marching into volumes, sharded
 * anything, device-side ray generation with lens jitter. */
int bt_scene_set_camera_focus(bt_scene *scene, uint64_t camera_ref, int has_focus, float focus);

void bt_tuning_default(bt_tuning *out);
/* NULL restores the defaults.  Returns BT_ERR_INVALID_ARG for a value outside the sets above. */
int bt_scene_set_tuning(bt_scene *scene, const bt_tuning *tuning);
int bt_scene_get_tuning(const bt_scene *scene, bt_tuning *out);

/* Returns the device memory a handle keeps between calls -- the parked sample values of the work queue (bt_stats.scratch_bytes;
 * it otherwise shrinks only after eight consecutive renders that needed less than a quarter of it) and bt_render's cached copy
 * of the caller's frame -- to the device (synchronises it).  The reference holds no such state: `Tracer::render` borrows the
 * scene and the buffer for the call (tracer/mod.rs:179-185).  A handle serves ONE stream at a time, like `&mut Buffer`. */
int bt_scene_trim(bt_scene *scene);

/* Work counters of the most recent bt_render* call on this handle (synchronises). */
int bt_scene_last_stats(bt_scene *scene, bt_stats *out);

#ifdef __cplusplus
}
#endif
#endif
