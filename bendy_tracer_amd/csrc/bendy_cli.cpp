// bendy_cli.cpp -- headless counterpart of the reference's viewer (src/main.rs), over the C ABI.
//
// Same flags as the clap `Cli` (main.rs:49-72): --width 768 --height 512 --output <full|albedo|normal>
// (required) --samples 64 --subsample 2 --screenshot screenshots/render.png --scene scene.json.
// The reference opens a minifb window unconditionally (main.rs:79-87) and reacts to Ctrl+P / Ctrl+K;
// without a display this program runs the same progressive loop (one `Tracer::render` call of
// 1 x subsample^2 rays per pixel per iteration until --samples is reached, main.rs:245-254), keeps
// the frame in HBM, prints what the window title would show (main.rs:352-388) and then does what
// Ctrl+P does (preview -> PNG, main.rs:275-298) and, with --save-scene, what Ctrl+K does
// (pretty JSON, gzip for .gz, main.rs:299-313).  Extra flags: --seed, --save-scene, --device, --quiet, and
// --lens x,y,z,rs,step,radius[,max_steps] for the gravitational-lens EXTENSION (not in the reference; bt_lens), and
// --denoise [--denoise-guide-samples N] for the denoiser EXTENSION (not in the reference; bt_denoiser): after the loop the
// albedo, normal and depth AOVs are rendered with N x subsample^2 rays per pixel (same seed) and the screenshot is the
// denoised mean.  --denoise-inline (extension too; bt_render_guided_device): every call of the progressive loop renders the colour
// AND the three guides in one pass into four device frames, and the screenshot is the denoised mean of those.
// --adaptive THRESHOLD [--adaptive-min N] [--adaptive-map PATH] (extension too; bt_adaptive): every call is one adaptive pass of
// --samples-per-call samples into the 16x16 tiles whose error estimate is still above THRESHOLD, --samples is the cap per tile,
// the loop ends when no tile is active; the screenshot (and what --denoise filters) is the resolved mean.
// --temporal [--frames N] [--camera-step X,Y,Z] (extension too; bt_temporal): N displayed frames; each clears the colour and guide
// frames, renders --samples x subsample^2 rays per pixel through the guided pass and accumulates them into the history
// reprojected from the frame before; the camera moves by the world-space step X,Y,Z before every frame after the first.  The
// screenshot is the last frame's accumulated mean (with --denoise: filtered with that frame's own guides).
// --tonemap clip|reinhard|aces, --exposure auto|EV [--exposure-key K] [--exposure-adapt A] [--white W] (extension too; bt_display):
// with any of them the screenshot comes from bt_display_device instead of bt_preview_device, applied to whatever frame is shown;
// under --temporal the stage runs once per displayed frame, so the exposure adapts across the frames.  --hdr PATH.pfm
// (bt_write_pfm) saves the linear mean of the frame that is shown.
// --glare STRENGTH [--glare-levels N] [--glare-spread X] (extension too; bt_glare): the mean that is about to be shown (plain,
// denoised, adaptive-resolved or temporal) passes bt_glare_device first, ahead of bt_display_device or bt_preview_device; under
// --temporal once per displayed frame.  --hdr then holds the glared mean, because that is what is shown.
// --resample WxH [--resample-filter box|tent|mitchell|lanczos3] (extension too; bt_resample): the mean that is about to be shown
// (plain, denoised, adaptive-resolved, temporal, glared) passes bt_resample_device last, ahead of bt_display_device or
// bt_preview_device; under --temporal once per displayed frame.  The screenshot and --hdr then have W x H pixels.
// --despeckle RATIO [--despeckle-rank K] [--despeckle-radius R] (extension too; bt_despeckle): the colour sums pass
// bt_despeckle_device right after the render and before everything else -- under --temporal each frame's sums before the
// accumulate, with --adaptive the resolved mean (n = 1), because tiles hold different counts.
// --upscale WxH [--upscale-guide-samples N] (extension too; bt_upscale): the camera aspect is W / H for every render; the
// progressive loop renders colour and guides at --width x --height through bt_render_guided_device; after it three
// bt_render_device calls render albedo, normal and depth at W x H (N samples, the same subsample), and the mean that is about to
// be shown (plain, despeckled, denoised in-line) passes bt_upscale_device ahead of the glare and the display stage.  The
// screenshot and --hdr then have W x H pixels; --stats-json gains an `upscale` object.
// --compare TRUTH.pfm [--compare-tail F] [--compare-map PATH.png [--compare-map-scale S]] (extension too; bt_compare): the
// scene-linear mean that --hdr would write -- after every stage, before the display stage -- is measured against the file, which
// must have the shown frame's size: MSE, relMSE, PSNR, SSIM, the largest difference, and the share of the error carried by the worst
// F (0.01 unless told) of the pixels.  The figures are printed and --stats-json gains a `compare` object; --compare-map saves the
// error plane in false colour, white at S (1 unless told).  It changes no output.
// --pick X,Y and --autofocus X,Y (extension too; bt_scene_pick, bt_scene_set_camera_focus): what the ray through the centre of
// pixel (X, Y) of the --width x --height frame hits, before the first render.  --pick prints one JSON line {"pick": {...}} to
// stdout ({"pick": null} for a miss) and --stats-json gains the same object; --autofocus sets the camera's focus to the pick's,
// so that the hit point lies in the focal plane of every render that follows (a miss is an error).  Not with --lens or --shard.
#include <hip/hip_runtime.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/bendy_hip.h"

namespace {

[[noreturn]] void die(const std::string &msg) {
    std::fprintf(stderr, "error: %s\n", msg.c_str());
    std::exit(1);
}
void check(int rc, const char *what) {
    if (rc < 0) die(std::string(what) + ": " + bt_last_error());
}
void hip_check(hipError_t e, const char *what) {
    if (e != hipSuccess) die(std::string(what) + ": " + hipGetErrorString(e));
}
bool exists(const std::string &p) {
    struct stat st;
    return ::stat(p.c_str(), &st) == 0;
}
bool is_dir(const std::string &p) {
    struct stat st;
    return ::stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}
void create_dir_all(const std::string &dir) {            // fs::create_dir_all, main.rs:292
    std::string cur;
    for (size_t i = 0; i <= dir.size(); ++i) {
        if (i == dir.size() || dir[i] == '/') {
            if (!cur.empty() && !exists(cur) && ::mkdir(cur.c_str(), 0777) != 0) die("cannot create directory " + cur);
        }
        if (i < dir.size()) cur += dir[i];
    }
}
std::string fmt_duration(double seconds) {               // main.rs:364-386
    long total_ms = (long)(seconds * 1000.0);
    long s = total_ms / 1000, ms = total_ms % 1000;
    char buf[64];
    if (s == 0) std::snprintf(buf, sizeof buf, "%ldms", ms);
    else std::snprintf(buf, sizeof buf, "%lds %ldms", s, ms);
    return buf;
}

struct Args {
    unsigned width = 768, height = 512;                  // main.rs:51-55
    std::string output;                                  // required, main.rs:57-58
    unsigned samples = 64, subsample = 2;                // main.rs:60-64
    std::string screenshot = "screenshots/render.png";   // main.rs:66-67
    std::string scene = "scene.json";                    // main.rs:69-70
    unsigned long long seed = 0x5EED;
    std::string save_scene;
    int device = 0;
    bool quiet = false;
    unsigned samples_per_call = 1;                       // main.rs:248 renders 1 sample per displayed frame
    bool no_screenshot = false;
    std::string stats_json;                              // per-call kernel times / segment counts (profiling harness)
    unsigned shard_rank = 0, shard_world = 1;            // --shard r,w: render rank r's tile shard of a w-rank job (measurement
                                                         // harness for bench.py --gpus N; no screenshot, the shard is tile-major)
    bool has_lens = false;
    bt_lens lens{};
    bool denoise = false;
    unsigned denoise_guide_samples = 4;
    bool denoise_inline = false;
    bool adaptive = false;
    float adaptive_threshold = 0.0f;
    long adaptive_min = -1;                               // -1: bt_adaptive_params_default's
    std::string adaptive_map;
    bool temporal = false;
    long frames = -1;                                     // -1: not given (1 with --temporal)
    bool has_camera_step = false;
    float camera_step[3] = {0.0f, 0.0f, 0.0f};
    bool display = false;                                 // any of --tonemap, --exposure, --exposure-key, --exposure-adapt, --white
    std::string tonemap = "aces";
    bool exposure_auto = true;
    float exposure_ev = 0.0f;
    double exposure_key = -1.0;                           // -1: bt_display_params_default's, as the next two
    float exposure_adapt = -1.0f, white = -1.0f;
    std::string hdr;
    bool glare = false;
    float glare_strength = 0.0f, glare_spread = -1.0f;   // -1: bt_glare_params_default's, as the levels
    long glare_levels = -1;
    bool resample = false;
    unsigned resample_width = 0, resample_height = 0;
    std::string resample_filter;                          // empty: not given (mitchell)
    bool despeckle = false;
    float despeckle_ratio = 0.0f;
    long despeckle_rank = -1, despeckle_radius = -1;      // -1: bt_despeckle_params_default's
    bool upscale = false;
    unsigned upscale_width = 0, upscale_height = 0;
    std::string compare, compare_map;                    // --compare TRUTH.pfm, --compare-map PATH.png
    double compare_tail = -1.0;                          // < 0: not given (0.01)
    float compare_map_scale = -1.0f;                     // < 0: not given (1)
    bool pick = false, autofocus = false;                // --pick X,Y, --autofocus X,Y
    unsigned pick_x = 0, pick_y = 0, autofocus_x = 0, autofocus_y = 0;
    long upscale_guide_samples = -1;                      // -1: not given (1)
};

void usage() {
    std::fprintf(stderr,
                 "usage: bendy-tracer-hip --output <full|albedo|normal> [--width 768] [--height 512] [--samples 64]\n"
                 "       [--subsample 2] [--screenshot screenshots/render.png] [--scene scene.json]\n"
                 "       [--seed N] [--save-scene PATH] [--device N] [--quiet]\n"
                 "       [--samples-per-call 1] [--no-screenshot] [--stats-json PATH] [--shard rank,world]   (measurement harness)\n"
                 "       [--lens x,y,z,rs,step,radius[,max_steps]]   (extension: not in the reference)\n"
                 "       [--denoise] [--denoise-guide-samples 4]   (extension: not in the reference; --output full only)\n"
                 "       [--denoise-inline]   (extension: colour and guides in one pass per call; --output full only, not with\n"
                 "                             --denoise, --shard or --lens)\n"
                 "       [--adaptive THRESHOLD] [--adaptive-min N] [--adaptive-map PATH]   (extension: adaptive sampling; --samples is\n"
                 "                             the cap, --samples-per-call the pass; --output full only, not with --lens, --shard\n"
                 "                             or --denoise-inline)\n"
                 "       [--temporal] [--frames N] [--camera-step X,Y,Z]   (extension: temporal accumulation with reprojection; N frames\n"
                 "                             of --samples each, the camera moved by X,Y,Z before each frame after the first;\n"
                 "                             --output full only, not with --lens, --shard, --adaptive or --denoise-inline)\n"
                 "       [--tonemap clip|reinhard|aces] [--exposure auto|EV] [--exposure-key 0.18] [--exposure-adapt 1] [--white 4]\n"
                 "                            (extension: display stage -- metered auto-exposure and a tone curve for the screenshot;\n"
                 "                             under --temporal the exposure adapts from frame to frame; --output full only, not\n"
                 "                             with --shard)\n"
                 "       [--hdr PATH.pfm]     (extension: the linear mean of the shown frame as a Portable Float Map; --output full\n"
                 "                             only, not with --shard)\n"
                 "       [--glare STRENGTH] [--glare-levels 6] [--glare-spread 1]   (extension: glare stage -- an energy-conserving bloom\n"
                 "                             on the mean that is shown, ahead of the display stage or the preview; --hdr then holds\n"
                 "                             the glared mean; --output full only, not with --shard)\n"
                 "       [--resample WxH] [--resample-filter box|tent|mitchell|lanczos3]   (extension: resample stage -- the mean that is\n"
                 "                             shown is filtered to W x H last, ahead of the display stage or the preview; the\n"
                 "                             screenshot and --hdr then have that size; mitchell unless told; --output full only,\n"
                 "                             not with --shard)\n"
                 "       [--despeckle RATIO] [--despeckle-rank 2] [--despeckle-radius 1]   (extension: despeckle stage -- a pixel brighter\n"
                 "                             than RATIO times the rank-th brightest of its neighbours is pulled down to that, on the\n"
                 "                             colour sums right after the render and before every other stage; --output full only,\n"
                 "                             not with --shard)\n"
                 "       [--upscale WxH] [--upscale-guide-samples 1]   (extension: upscale stage -- the render of --width x --height is shown at\n"
                 "                             W x H, every texel weighed by how well its albedo, normal and depth match those of a\n"
                 "                             guide-only render of N samples at W x H; after --despeckle and --denoise-inline, before\n"
                 "                             --glare and the display stage; the screenshot and --hdr then have W x H pixels; --output\n"
                 "                             full only, not with --shard, --lens, --resample, --denoise, --adaptive or --temporal)\n"
                 "       [--compare TRUTH.pfm] [--compare-tail 0.01] [--compare-map PATH.png] [--compare-map-scale 1]\n"
                 "                            (extension: MSE, relMSE, PSNR, SSIM and the tail share of the frame --hdr would write\n"
                 "                             against a PFM of the same size; --output full only, not with --shard)\n"
                 "       [--pick X,Y] [--autofocus X,Y]\n"
                 "                            (extension: what the ray through pixel (X, Y) hits, as one JSON line; the camera focus\n"
                 "                             that puts it in the focal plane, set before the first render; not with --lens, --shard)\n");
}

Args parse(int argc, char **argv) {
    Args a;
    for (int i = 1; i < argc; ++i) {
        std::string k = argv[i], v;
        size_t eq = k.find('=');
        bool has_v = false;
        if (eq != std::string::npos) { v = k.substr(eq + 1); k = k.substr(0, eq); has_v = true; }
        auto val = [&]() -> std::string {
            if (has_v) return v;
            if (i + 1 >= argc) { usage(); die("missing value for " + k); }
            return argv[++i];
        };
        if (k == "--width") a.width = (unsigned)std::strtoul(val().c_str(), nullptr, 10);
        else if (k == "--height") a.height = (unsigned)std::strtoul(val().c_str(), nullptr, 10);
        else if (k == "--output") a.output = val();
        else if (k == "--samples") a.samples = (unsigned)std::strtoul(val().c_str(), nullptr, 10);
        else if (k == "--subsample") a.subsample = (unsigned)std::strtoul(val().c_str(), nullptr, 10);
        else if (k == "--screenshot") a.screenshot = val();
        else if (k == "--scene") a.scene = val();
        else if (k == "--seed") a.seed = std::strtoull(val().c_str(), nullptr, 0);
        else if (k == "--save-scene") a.save_scene = val();
        else if (k == "--device") a.device = std::atoi(val().c_str());
        else if (k == "--quiet") a.quiet = true;
        else if (k == "--samples-per-call") a.samples_per_call = std::max(1u, (unsigned)std::strtoul(val().c_str(), nullptr, 10));
        else if (k == "--no-screenshot") a.no_screenshot = true;
        else if (k == "--stats-json") a.stats_json = val();
        else if (k == "--shard") {
            const std::string spec = val();
            if (std::sscanf(spec.c_str(), "%u,%u", &a.shard_rank, &a.shard_world) != 2 || a.shard_world == 0 || a.shard_rank >= a.shard_world)
                die("--shard expects rank,world with rank < world");
            a.no_screenshot = true;
        }
        else if (k == "--lens") {
            const std::string spec = val();
            float f[7] = {0, 0, 0, 0, 0, 0, 4096};
            int n = std::sscanf(spec.c_str(), "%f,%f,%f,%f,%f,%f,%f", &f[0], &f[1], &f[2], &f[3], &f[4], &f[5], &f[6]);
            if (n < 6) die("--lens expects x,y,z,rs,step,radius[,max_steps]");
            a.lens.centre[0] = f[0]; a.lens.centre[1] = f[1]; a.lens.centre[2] = f[2];
            a.lens.rs = f[3]; a.lens.step = f[4]; a.lens.radius = f[5];
            a.lens.max_steps = (uint32_t)f[6];
            a.has_lens = true;
        }
        else if (k == "--denoise") a.denoise = true;
        else if (k == "--denoise-inline") a.denoise_inline = true;
        else if (k == "--denoise-guide-samples") a.denoise_guide_samples = (unsigned)std::strtoul(val().c_str(), nullptr, 10);
        else if (k == "--adaptive") {
            const std::string spec = val();
            char *end = nullptr;
            a.adaptive_threshold = std::strtof(spec.c_str(), &end);
            if (spec.empty() || *end != 0 || !(a.adaptive_threshold >= 0.0f) || !(a.adaptive_threshold < 3.0e38f))
                die("--adaptive expects a finite threshold >= 0");
            a.adaptive = true;
        }
        else if (k == "--adaptive-min") a.adaptive_min = (long)std::strtoul(val().c_str(), nullptr, 10);
        else if (k == "--adaptive-map") a.adaptive_map = val();
        else if (k == "--temporal") a.temporal = true;
        else if (k == "--frames") {
            const std::string spec = val();
            char *end = nullptr;
            a.frames = std::strtol(spec.c_str(), &end, 10);
            if (spec.empty() || *end != 0 || a.frames < 1 || a.frames > 1000000) die("--frames expects a count >= 1");
        }
        else if (k == "--camera-step") {
            const std::string spec = val();
            char tail = 0;
            if (std::sscanf(spec.c_str(), "%f,%f,%f%c", &a.camera_step[0], &a.camera_step[1], &a.camera_step[2], &tail) != 3 ||
                !(std::fabs(a.camera_step[0]) < 3.0e38f) || !(std::fabs(a.camera_step[1]) < 3.0e38f) || !(std::fabs(a.camera_step[2]) < 3.0e38f))
                die("--camera-step expects X,Y,Z (finite)");
            a.has_camera_step = true;
        }
        else if (k == "--tonemap") {
            a.tonemap = val();
            if (a.tonemap != "clip" && a.tonemap != "reinhard" && a.tonemap != "aces") die("--tonemap expects clip, reinhard or aces");
            a.display = true;
        }
        else if (k == "--exposure") {
            const std::string spec = val();
            a.exposure_auto = spec == "auto";
            if (!a.exposure_auto) {
                char *end = nullptr;
                a.exposure_ev = std::strtof(spec.c_str(), &end);
                if (spec.empty() || *end != 0 || !(std::fabs(a.exposure_ev) < 3.0e38f)) die("--exposure expects auto or a finite EV");
            }
            a.display = true;
        }
        else if (k == "--exposure-key" || k == "--exposure-adapt" || k == "--white") {
            const std::string spec = val();
            char *end = nullptr;
            const double f = std::strtod(spec.c_str(), &end);
            const bool ok = !spec.empty() && *end == 0 && f > 0.0 && f < 3.0e38;
            if (k == "--exposure-key") { if (!ok) die("--exposure-key expects a finite value > 0"); a.exposure_key = f; }
            else if (k == "--exposure-adapt") { if (!ok || f > 1.0) die("--exposure-adapt expects a value in (0, 1]"); a.exposure_adapt = (float)f; }
            else { if (!ok) die("--white expects a finite value > 0"); a.white = (float)f; }
            a.display = true;
        }
        else if (k == "--hdr") a.hdr = val();
        else if (k == "--glare" || k == "--glare-spread") {
            const std::string spec = val();
            char *end = nullptr;
            const float f = std::strtof(spec.c_str(), &end);
            const bool ok = !spec.empty() && *end == 0;
            if (k == "--glare") {
                if (!ok || !(f >= 0.0f && f <= 1.0f)) die("--glare expects a strength in [0, 1]");
                a.glare_strength = f;
                a.glare = true;
            } else {
                if (!ok || !(f > 0.0f && f <= 16.0f)) die("--glare-spread expects a value in (0, 16]");
                a.glare_spread = f;
            }
        }
        else if (k == "--glare-levels") {
            const std::string spec = val();
            char *end = nullptr;
            a.glare_levels = std::strtol(spec.c_str(), &end, 10);
            if (spec.empty() || *end != 0 || a.glare_levels < 0 || a.glare_levels > 16) die("--glare-levels expects a count in 0 .. 16");
        }
        else if (k == "--resample") {
            const std::string spec = val();
            char tail = 0;
            if (std::sscanf(spec.c_str(), "%ux%u%c", &a.resample_width, &a.resample_height, &tail) != 2 || spec[0] < '0' || spec[0] > '9' ||
                a.resample_width == 0 || a.resample_height == 0 || a.resample_width > 0x7fffffffu || a.resample_height > 0x7fffffffu)
                die("--resample expects WxH, both positive");
            a.resample = true;
        }
        else if (k == "--resample-filter") {
            a.resample_filter = val();
            if (a.resample_filter != "box" && a.resample_filter != "tent" && a.resample_filter != "mitchell" && a.resample_filter != "lanczos3")
                die("--resample-filter expects box, tent, mitchell or lanczos3");
        }
        else if (k == "--despeckle") {
            const std::string spec = val();
            char *end = nullptr;
            a.despeckle_ratio = std::strtof(spec.c_str(), &end);
            if (spec.empty() || *end != 0 || !(a.despeckle_ratio >= 1.0f) || !(a.despeckle_ratio < 3.0e38f))
                die("--despeckle expects a finite ratio >= 1");
            a.despeckle = true;
        }
        else if (k == "--despeckle-rank" || k == "--despeckle-radius") {
            const std::string spec = val();
            char *end = nullptr;
            const long n = std::strtol(spec.c_str(), &end, 10);
            const bool ok = !spec.empty() && *end == 0;
            if (k == "--despeckle-rank") {
                if (!ok || n < 1 || n > 24) die("--despeckle-rank expects a count in 1 .. 24");
                a.despeckle_rank = n;
            } else {
                if (!ok || (n != 1 && n != 2)) die("--despeckle-radius expects 1 or 2");
                a.despeckle_radius = n;
            }
        }
        else if (k == "--upscale") {
            const std::string spec = val();
            char tail = 0;
            if (std::sscanf(spec.c_str(), "%ux%u%c", &a.upscale_width, &a.upscale_height, &tail) != 2 || spec[0] < '0' || spec[0] > '9' ||
                a.upscale_width == 0 || a.upscale_height == 0 || a.upscale_width > 0x7fffffffu || a.upscale_height > 0x7fffffffu)
                die("--upscale expects WxH, both positive");
            a.upscale = true;
        }
        else if (k == "--upscale-guide-samples") {
            const std::string spec = val();
            char *end = nullptr;
            a.upscale_guide_samples = std::strtol(spec.c_str(), &end, 10);
            if (spec.empty() || *end != 0 || a.upscale_guide_samples < 1 || a.upscale_guide_samples > 0xffff)
                die("--upscale-guide-samples expects a count in 1 .. 65535");
        }
        else if (k == "--pick" || k == "--autofocus") {
            const std::string spec = val();
            unsigned x = 0, y = 0;
            char tail = 0;
            if (std::sscanf(spec.c_str(), "%u,%u%c", &x, &y, &tail) != 2 || spec[0] == '-') die(k + " expects X,Y");
            if (k == "--pick") { a.pick = true; a.pick_x = x; a.pick_y = y; }
            else { a.autofocus = true; a.autofocus_x = x; a.autofocus_y = y; }
        }
        else if (k == "--compare") a.compare = val();
        else if (k == "--compare-map") a.compare_map = val();
        else if (k == "--compare-tail") {
            const std::string spec = val();
            char *end = nullptr;
            a.compare_tail = std::strtod(spec.c_str(), &end);
            if (spec.empty() || *end != 0 || !(a.compare_tail > 0.0 && a.compare_tail <= 1.0)) die("--compare-tail expects a fraction in (0, 1]");
        }
        else if (k == "--compare-map-scale") {
            const std::string spec = val();
            char *end = nullptr;
            a.compare_map_scale = std::strtof(spec.c_str(), &end);
            if (spec.empty() || *end != 0 || !(a.compare_map_scale > 0.0f && a.compare_map_scale < 3.0e38f)) die("--compare-map-scale expects a finite value > 0");
        }
        else if (k == "--help" || k == "-h") { usage(); std::exit(0); }
        else { usage(); die("unknown argument " + k); }
    }
    if (a.output.empty()) { usage(); die("the following required arguments were not provided: --output <OUTPUT>"); }
    if (a.width == 0 || a.height == 0) die("width and height must be positive");
    if (a.denoise && a.output != "full") die("--denoise needs --output full");
    if (a.denoise && a.shard_world > 1) die("--denoise does not apply to a --shard run");
    if (a.denoise && a.denoise_guide_samples == 0) die("--denoise-guide-samples must be positive");
    if (a.denoise_inline && a.output != "full") die("--denoise-inline needs --output full");
    if (a.denoise_inline && a.denoise) die("--denoise-inline and --denoise exclude each other");
    if (a.denoise_inline && a.shard_world > 1) die("--denoise-inline does not apply to a --shard run");
    if (a.denoise_inline && a.has_lens) die("--denoise-inline has no builds for --lens");
    if (!a.adaptive && (a.adaptive_min >= 0 || !a.adaptive_map.empty())) die("--adaptive-min and --adaptive-map need --adaptive");
    if (a.adaptive && a.output != "full") die("--adaptive needs --output full");
    if (a.adaptive && a.has_lens) die("--adaptive has no builds for --lens");
    if (a.adaptive && a.shard_world > 1) die("--adaptive does not apply to a --shard run");
    if (a.adaptive && a.denoise_inline) die("--adaptive has no guided variant: use --denoise, not --denoise-inline");
    if (a.adaptive && a.adaptive_min > (long)a.samples) die("--adaptive-min must not exceed --samples (the cap)");
    if (!a.temporal && (a.frames >= 0 || a.has_camera_step)) die("--frames and --camera-step need --temporal");
    if (a.temporal && a.output != "full") die("--temporal needs --output full");
    if (a.temporal && a.has_lens) die("--temporal has no inverse map for --lens");
    if (a.temporal && a.shard_world > 1) die("--temporal does not apply to a --shard run");
    if (a.temporal && a.adaptive) die("--temporal does not take the frames of --adaptive, whose tiles hold different counts");
    if (a.temporal && a.denoise_inline) die("--temporal renders its own guides: use --denoise, not --denoise-inline");
    if (a.temporal && a.samples == 0) die("--temporal needs --samples >= 1 per frame");
    if (a.temporal && a.frames < 0) a.frames = 1;
    if (a.display && a.output != "full") die("--tonemap and --exposure need --output full");
    if (a.display && a.shard_world > 1) die("--tonemap and --exposure do not apply to a --shard run");
    if (!a.hdr.empty() && a.output != "full") die("--hdr needs --output full");
    if (!a.hdr.empty() && a.shard_world > 1) die("--hdr does not apply to a --shard run");
    if (!a.glare && (a.glare_levels >= 0 || a.glare_spread > 0.0f)) die("--glare-levels and --glare-spread need --glare");
    if (a.glare && a.output != "full") die("--glare needs --output full");
    if (a.glare && a.shard_world > 1) die("--glare does not apply to a --shard run");
    if (!a.resample && !a.resample_filter.empty()) die("--resample-filter needs --resample");
    if (a.resample && a.output != "full") die("--resample needs --output full");
    if (a.resample && a.shard_world > 1) die("--resample does not apply to a --shard run");
    if (!a.despeckle && (a.despeckle_rank >= 0 || a.despeckle_radius >= 0)) die("--despeckle-rank and --despeckle-radius need --despeckle");
    if (a.despeckle && a.output != "full") die("--despeckle needs --output full");
    if (a.despeckle && a.shard_world > 1) die("--despeckle does not apply to a --shard run");
    if (a.despeckle && a.despeckle_rank > (a.despeckle_radius == 2 ? 24 : 8))
        die("--despeckle-rank must not exceed the window's neighbours: 8 at radius 1, 24 at --despeckle-radius 2");
    if (!a.upscale && a.upscale_guide_samples >= 0) die("--upscale-guide-samples needs --upscale");
    if (a.upscale && a.output != "full") die("--upscale needs --output full");
    if (a.upscale && a.shard_world > 1) die("--upscale does not apply to a --shard run");
    if (a.upscale && a.has_lens) die("--upscale renders its guides in one pass with the colour, which has no builds for --lens");
    if (a.upscale && a.resample) die("--upscale and --resample exclude each other: one frame is shown at one size");
    if (a.upscale && a.denoise) die("--upscale takes the guides of the colour pass: use --denoise-inline, not --denoise");
    if (a.upscale && a.adaptive) die("--upscale does not take the frames of --adaptive, which has no guided variant");
    if (a.upscale && a.temporal) die("--upscale does not apply to a --temporal run");
    if (a.upscale && (a.upscale_width < a.width || a.upscale_height < a.height))
        die("--upscale must not be smaller than --width x --height on either axis: --resample reduces");
    for (int which = 0; which < 2; ++which) {
        if (!(which ? a.autofocus : a.pick)) continue;
        const std::string name = which ? "--autofocus" : "--pick";
        const unsigned x = which ? a.autofocus_x : a.pick_x, y = which ? a.autofocus_y : a.pick_y;
        if (x >= a.width || y >= a.height)
            die(name + ": pixel (" + std::to_string(x) + ", " + std::to_string(y) + ") is outside the " + std::to_string(a.width) + "x" + std::to_string(a.height) + " frame");
        if (a.has_lens) die(name + " sends a straight ray: not with --lens");
        if (a.shard_world > 1) die(name + " does not apply to a --shard run");
    }
    if (a.compare.empty() && (a.compare_tail >= 0.0 || !a.compare_map.empty() || a.compare_map_scale >= 0.0f))
        die("--compare-tail, --compare-map and --compare-map-scale need --compare");
    if (a.compare_map.empty() && a.compare_map_scale >= 0.0f) die("--compare-map-scale needs --compare-map");
    if (!a.compare.empty() && a.output != "full") die("--compare needs --output full");
    if (!a.compare.empty() && a.shard_world > 1) die("--compare does not apply to a --shard run");
    if (!a.compare.empty()) {                            // the file's size against the shown frame's, before any device work
        const unsigned sw = a.resample ? a.resample_width : a.upscale ? a.upscale_width : a.width;
        const unsigned sh = a.resample ? a.resample_height : a.upscale ? a.upscale_height : a.height;
        uint32_t tw = 0, th = 0;
        if (bt_read_pfm(a.compare.c_str(), nullptr, 0, &tw, &th) < 0) die(std::string("--compare: ") + bt_last_error());
        if (tw != sw || th != sh)
            die("--compare: " + a.compare + " has " + std::to_string(tw) + "x" + std::to_string(th) + " pixels, the shown frame " + std::to_string(sw) +
                "x" + std::to_string(sh));
    }
    return a;
}

} // namespace

int main(int argc, char **argv) {
    const Args args = parse(argc, argv);
    // main.rs:23-47: CLI Output -> tracer Output + ColorSpace
    int output, color_space;
    if (args.output == "full") { output = BT_OUTPUT_FULL; color_space = BT_COLOR_SRGB; }
    else if (args.output == "albedo") { output = BT_OUTPUT_ALBEDO; color_space = BT_COLOR_SRGB; }
    else if (args.output == "normal") { output = BT_OUTPUT_NORMAL; color_space = BT_COLOR_NORMAL; }
    else die("invalid value '" + args.output + "' for '--output <OUTPUT>' [possible values: full, albedo, normal]");

    hip_check(hipSetDevice(args.device), "hipSetDevice");

    // main.rs:93-214: load the scene if the file exists, else the built-in Cornell scene
    bt_scene *scene;
    if (exists(args.scene)) {
        scene = bt_scene_load(args.scene.c_str());
        if (!scene) die(bt_last_error());
        std::fprintf(stderr, "loaded scene from %s\n", args.scene.c_str());
    } else {
        scene = bt_scene_default();
        if (!scene) die(bt_last_error());
    }
    uint64_t camera = 0;
    check(bt_scene_find_by_tag(scene, "camera", &camera), "find_by_tag(\"camera\")");          // main.rs:216
    // :218-223; under --upscale every render, small or large, shows the frame of the shown size
    check(bt_scene_set_camera_aspect(scene, camera, args.upscale ? (float)args.upscale_width / (float)args.upscale_height
                                                                  : (float)args.width / (float)args.height), "aspect");
    if (args.has_lens) check(bt_scene_set_lens(scene, &args.lens), "bt_scene_set_lens");
    {
        // measurement harness: launch-shape knobs from the environment (the LIBRARY never reads it; this tool does, like
        // tools/*.py through Scene.tuning_from_env)
        bt_tuning t;
        bt_tuning_default(&t);
        bool any = false;
        auto env = [&](const char *name, auto &field) {
            if (const char *e = std::getenv(name)) { field = (std::remove_reference_t<decltype(field)>)std::strtoll(e, nullptr, 10); any = true; }
        };
        env("BT_SLICES", t.slices); env("BT_PHASE_VOTE", t.phase_vote); env("BT_SCRATCH_CAP", t.scratch_cap_bytes); env("BT_PACKED", t.packed);
        if (any) check(bt_scene_set_tuning(scene, &t), "bt_scene_set_tuning");
    }

    bt_config cfg;
    bt_config_default(&cfg);
    cfg.output = output;
    cfg.chunks_x = 8;                                      // main.rs:225-230
    cfg.chunks_y = 4;
    bt_render_config rc;
    bt_render_config_default(&rc);
    rc.subsample_n = args.subsample <= 1 ? 0 : args.subsample;   // main.rs:234-237
    const unsigned nn = rc.subsample_n ? rc.subsample_n * rc.subsample_n : 1;

    // --pick / --autofocus (extension): before anything is rendered
    std::string pick_json;
    if (args.pick) {
        bt_hit hit{};
        float focus = 0.0f;
        const int found = bt_scene_pick(scene, camera, &cfg, &rc, args.width, args.height, args.pick_x, args.pick_y, &hit, &focus);
        check(found, "bt_scene_pick");
        char pj[640] = "\"pick\": null";
        if (found) {
            char vol[32] = "null";
            if (hit.volume_ref != UINT64_MAX) std::snprintf(vol, sizeof vol, "%llu", (unsigned long long)hit.volume_ref);
            std::snprintf(pj, sizeof pj, "\"pick\": {\"position\": [%.9g, %.9g, %.9g], \"t\": %.9g, \"normal\": [%.9g, %.9g, %.9g], "
                          "\"face\": %d, \"object_ref\": %llu, \"material_ref\": %llu, \"volume_ref\": %s, \"prim\": %d, \"focus\": %.9g}",
                          hit.position[0], hit.position[1], hit.position[2], hit.t, hit.normal[0], hit.normal[1], hit.normal[2], hit.face,
                          (unsigned long long)hit.object_ref, (unsigned long long)hit.material_ref, vol, hit.prim, focus);
        }
        std::printf("{%s}\n", pj);
        std::fflush(stdout);
        pick_json = std::string(", ") + pj;
    }
    if (args.autofocus) {
        bt_hit hit{};
        float focus = 0.0f;
        const int found = bt_scene_pick(scene, camera, &cfg, &rc, args.width, args.height, args.autofocus_x, args.autofocus_y, &hit, &focus);
        check(found, "bt_scene_pick");
        if (!found)
            die("--autofocus: the ray through pixel (" + std::to_string(args.autofocus_x) + ", " + std::to_string(args.autofocus_y) + ") hits nothing");
        check(bt_scene_set_camera_focus(scene, camera, 1, focus), "bt_scene_set_camera_focus");
        if (!args.quiet) std::fprintf(stderr, "autofocus: pixel (%u, %u) is %.6g away, focus %.6g\n", args.autofocus_x, args.autofocus_y, hit.t, focus);
    }

    // Buffer::new (buffer.rs:41-50), resident in HBM
    const bool sharded = args.shard_world > 1;
    const size_t n_px = sharded ? bt_shard_floats(args.width, args.height, args.shard_world) / 4 : (size_t)args.width * args.height;
    std::vector<float> init(n_px * 4, 0.0f);
    for (size_t i = 0; i < n_px; ++i) init[4 * i + 3] = 1.0f;
    float *d_frame = nullptr;
    uint8_t *d_rgba8 = nullptr;
    hip_check(hipMalloc((void **)&d_frame, n_px * 16), "hipMalloc");
    const size_t n_shown = args.resample  ? (size_t)args.resample_width * args.resample_height                  // the frame that is shown
                           : args.upscale ? (size_t)args.upscale_width * args.upscale_height
                                          : n_px;
    hip_check(hipMalloc((void **)&d_rgba8, n_shown * 4), "hipMalloc");
    hip_check(hipMemcpy(d_frame, init.data(), n_px * 16, hipMemcpyHostToDevice), "hipMemcpy");

    // --denoise-inline (extension): the guides' frames and the denoised mean; every call below fills all four in one pass
    float *d_guides[4] = {nullptr, nullptr, nullptr, nullptr};          // albedo, normal, depth, denoised mean
    if (args.denoise_inline || args.temporal || args.upscale)
        for (int g = 0; g < 4; ++g) {
            hip_check(hipMalloc((void **)&d_guides[g], n_px * 16), "hipMalloc");
            hip_check(hipMemcpy(d_guides[g], init.data(), n_px * 16, hipMemcpyHostToDevice), "hipMemcpy");
        }

    // main.rs:245-254: one sample per call while buffer.samples() < max_samples
    unsigned buffer_samples = 0;
    double sum_delta = 0.0;
    const auto start = std::chrono::steady_clock::now();
    std::string per_call;                                  // --stats-json rows
    // --adaptive (extension): passes of samples_per_call samples into the tiles still active, until none is
    bt_adaptive *adaptive = nullptr;
    bt_adaptive_stats astats{};
    float *d_mean = nullptr;                               // the resolved mean
    if (args.adaptive) {
        adaptive = bt_adaptive_new(args.width, args.height);
        if (!adaptive) die(bt_last_error());
        bt_adaptive_params ap;
        bt_adaptive_params_default(&ap);
        ap.threshold = args.adaptive_threshold;
        ap.max_samples = args.samples;
        ap.min_samples = args.adaptive_min >= 0 ? (uint32_t)args.adaptive_min : std::min(ap.min_samples, ap.max_samples);
        rc.samples = args.samples_per_call;
        for (;;) {
            const auto t0 = std::chrono::steady_clock::now();
            check(bt_render_adaptive_device(scene, camera, &cfg, &rc, adaptive, &ap, d_frame, args.width, args.height, args.seed, nullptr),
                  "bt_render_adaptive_device");
            const int st = bt_adaptive_poll(adaptive, &astats);
            check(st, "bt_adaptive_poll");
            const double delta = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            sum_delta += delta;
            buffer_samples = astats.max_count;
            if (!args.stats_json.empty()) {
                bt_stats cs{};
                bt_scene_last_stats(scene, &cs);
                char row[256];
                std::snprintf(row, sizeof row, "%s{\"kernel_ms\": %.5f, \"segments\": %llu, \"active_tiles\": %u, \"slices\": %u, \"packed\": %u}",
                              per_call.empty() ? "" : ", ", cs.kernel_ms, (unsigned long long)cs.segments, astats.active_tiles, cs.slices, cs.packed);
                per_call += row;
            }
            if (!args.quiet)
                std::fprintf(stderr, "bendy tracer; adaptive pass %u; samples: %u..%u/%u; active tiles: %u/%u; delta t: %s\n", astats.passes,
                             astats.min_count, astats.max_count, args.samples, astats.active_tiles, astats.tiles, fmt_duration(delta).c_str());
            if (st == BT_DONE) break;
        }
        hip_check(hipMalloc((void **)&d_mean, n_px * 16), "hipMalloc");
        check(bt_adaptive_resolve_device(adaptive, d_frame, d_mean, nullptr), "bt_adaptive_resolve_device");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    }
    // --tonemap / --exposure (extension): the display stage replaces the plain preview
    bt_display *display = nullptr;
    bt_display_params dp;
    bt_display_params_default(&dp);
    if (args.display) {
        display = bt_display_new();
        if (!display) die(bt_last_error());
        dp.tonemap = args.tonemap == "clip" ? BT_TONEMAP_CLIP : args.tonemap == "reinhard" ? BT_TONEMAP_REINHARD : BT_TONEMAP_ACES;
        dp.auto_exposure = args.exposure_auto ? 1 : 0;
        dp.ev = args.exposure_ev;
        if (args.exposure_key > 0.0) dp.key = args.exposure_key;
        if (args.exposure_adapt > 0.0f) dp.adapt = args.exposure_adapt;
        if (args.white > 0.0f) dp.white = args.white;
    }
    // --glare (extension): the mean that is shown passes the glare stage first
    bt_glare *glare = nullptr;
    bt_glare_params gp;
    bt_glare_params_default(&gp);
    float *d_glare = nullptr;                              // the glared mean
    std::string glare_json;
    uint32_t glare_levels = 0;                             // the effective number: bt_glare_device's step 2
    if (args.glare) {
        glare = bt_glare_new();
        if (!glare) die(bt_last_error());
        gp.strength = args.glare_strength;
        if (args.glare_levels >= 0) gp.levels = (uint32_t)args.glare_levels;
        if (args.glare_spread > 0.0f) gp.spread = args.glare_spread;
        hip_check(hipMalloc((void **)&d_glare, (args.upscale ? n_shown : n_px) * 16), "hipMalloc");
        for (uint32_t m = (args.upscale ? std::max(args.upscale_width, args.upscale_height) : std::max(args.width, args.height)) - 1; m; m >>= 1)
            ++glare_levels;
        glare_levels = std::min(glare_levels, gp.levels);
        char gj[160];
        std::snprintf(gj, sizeof gj, ", \"glare\": {\"strength\": %.9g, \"levels\": %u, \"spread\": %.9g}", gp.strength,
                      glare_levels, gp.spread);
        glare_json = gj;
    }
    // --resample (extension): the mean that is shown is filtered to another size last
    bt_resample *resample = nullptr;
    bt_resample_params rp;
    bt_resample_params_default(&rp);
    float *d_resampled = nullptr;                          // the resampled mean
    const unsigned shown_w = args.resample ? args.resample_width : args.upscale ? args.upscale_width : args.width;
    const unsigned shown_h = args.resample ? args.resample_height : args.upscale ? args.upscale_height : args.height;
    // the glare stage works on the frame the upscale stage hands on, and otherwise on the render
    const unsigned glare_w = args.upscale ? args.upscale_width : args.width, glare_h = args.upscale ? args.upscale_height : args.height;
    if (args.resample) {
        resample = bt_resample_new();
        if (!resample) die(bt_last_error());
        if (!args.resample_filter.empty())
            rp.filter = args.resample_filter == "box" ? BT_RESAMPLE_BOX : args.resample_filter == "tent" ? BT_RESAMPLE_TENT
                      : args.resample_filter == "mitchell" ? BT_RESAMPLE_MITCHELL : BT_RESAMPLE_LANCZOS3;
        hip_check(hipMalloc((void **)&d_resampled, n_shown * 16), "hipMalloc");
    }
    // --despeckle (extension): the colour sums pass the despeckle stage right after the render, before everything else
    bt_despeckle *despeckle = nullptr;
    bt_despeckle_params sp;
    bt_despeckle_params_default(&sp);
    bt_despeckle_stats sstats{};                           // of the last call
    float *d_despeckled = nullptr;                         // the despeckled sums
    if (args.despeckle) {
        despeckle = bt_despeckle_new();
        if (!despeckle) die(bt_last_error());
        sp.ratio = args.despeckle_ratio;
        if (args.despeckle_rank >= 0) sp.rank = (uint32_t)args.despeckle_rank;
        if (args.despeckle_radius >= 0) sp.radius = (uint32_t)args.despeckle_radius;
        hip_check(hipMalloc((void **)&d_despeckled, n_px * 16), "hipMalloc");
    }
    // --temporal (extension): one guided render into cleared frames and one accumulate per displayed frame
    bt_temporal *temporal = nullptr;
    double history_mean = 0.0, history_min = 0.0;
    if (args.temporal) {
        temporal = bt_temporal_new(args.width, args.height);
        if (!temporal) die(bt_last_error());
        hip_check(hipMalloc((void **)&d_mean, n_px * 16), "hipMalloc");
        rc.samples = args.samples;
        bt_view view;
        check(bt_scene_camera_view(scene, camera, &cfg, &rc, args.width, args.height, &view), "bt_scene_camera_view");
        for (long f = 0; f < args.frames; ++f) {
            const auto t0 = std::chrono::steady_clock::now();
            if (f > 0) {
                for (int k = 0; k < 3; ++k) view.to_world[9 + k] += args.camera_step[k];
                check(bt_scene_set_camera_pose(scene, camera, view.to_world), "bt_scene_set_camera_pose");
            }
            hip_check(hipMemcpy(d_frame, init.data(), n_px * 16, hipMemcpyHostToDevice), "hipMemcpy");
            for (int g = 0; g < 3; ++g) hip_check(hipMemcpy(d_guides[g], init.data(), n_px * 16, hipMemcpyHostToDevice), "hipMemcpy");
            rc.sample_base = (uint32_t)f * args.samples;   // fresh samples every frame
            check(bt_render_guided_device(scene, camera, &cfg, &rc, d_frame, d_guides[0], d_guides[1], d_guides[2], args.width,
                                          args.height, args.seed, nullptr),
                  "bt_render_guided_device");
            if (despeckle)                                  // this frame's sums, before they enter the history
                check(bt_despeckle_device(despeckle, d_frame, args.samples * nn, d_despeckled, args.width, args.height, &sp, nullptr),
                      "bt_despeckle_device");
            check(bt_temporal_accumulate_device(temporal, &view, despeckle ? d_despeckled : d_frame, args.samples * nn, d_guides[1], args.samples * nn, d_guides[2],
                                                args.samples * nn, d_mean, nullptr, nullptr),
                  "bt_temporal_accumulate_device");
            // every displayed frame passes the glare, the resample and the display stage; the last one does below, on the frame the
            // screenshot shows
            if (glare && f + 1 < args.frames)
                check(bt_glare_device(glare, d_mean, 1, d_glare, args.width, args.height, &gp, nullptr), "bt_glare_device");
            if (resample && f + 1 < args.frames)
                check(bt_resample_device(resample, glare ? d_glare : d_mean, 1, args.width, args.height, d_resampled, shown_w, shown_h, &rp,
                                         nullptr),
                      "bt_resample_device");
            if (display && f + 1 < args.frames)
                check(bt_display_device(display, resample ? d_resampled : glare ? d_glare : d_mean, 1, d_rgba8, shown_w, shown_h, color_space,
                                        &dp, nullptr),
                      "bt_display_device");
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
            const double delta = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            sum_delta += delta;
            buffer_samples += args.samples * nn;
            if (!args.stats_json.empty()) {
                bt_stats cs{};
                bt_scene_last_stats(scene, &cs);
                char row[256];
                std::snprintf(row, sizeof row, "%s{\"kernel_ms\": %.5f, \"segments\": %llu, \"samples\": %llu, \"pixels\": %llu, \"slices\": %u, \"packed\": %u}",
                              per_call.empty() ? "" : ", ", cs.kernel_ms, (unsigned long long)cs.segments,
                              (unsigned long long)cs.samples, (unsigned long long)cs.pixels, cs.slices, cs.packed);
                per_call += row;
            }
            if (!args.quiet)
                std::fprintf(stderr, "bendy tracer; temporal frame %ld/%ld; samples per frame: %u; delta t: %s\n", f + 1, args.frames,
                             args.samples * nn, fmt_duration(delta).c_str());
        }
        std::vector<float> hist(n_px * 4);
        check(bt_debug_temporal_history(temporal, hist.data(), (uint32_t)(n_px * 4)), "bt_debug_temporal_history");
        history_min = hist[3];
        for (size_t i = 0; i < n_px; ++i) {
            history_mean += hist[4 * i + 3];
            history_min = std::min(history_min, (double)hist[4 * i + 3]);
        }
        history_mean /= (double)n_px;
    }
    while (!args.adaptive && !args.temporal && buffer_samples < args.samples) {
        rc.samples = std::min(args.samples_per_call, std::max(1u, (args.samples - buffer_samples) / nn));
        rc.sample_base = (buffer_samples + nn - 1) / nn;
        const auto t0 = std::chrono::steady_clock::now();
        int st = args.denoise_inline || args.upscale
                     ? bt_render_guided_device(scene, camera, &cfg, &rc, d_frame, d_guides[0], d_guides[1], d_guides[2], args.width,
                                               args.height, args.seed, nullptr)
                 : sharded ? bt_render_shard_device(scene, camera, &cfg, &rc, d_frame, args.width, args.height, args.shard_rank,
                                                  args.shard_world, args.seed, nullptr)
                         : bt_render_device(scene, camera, &cfg, &rc, d_frame, args.width, args.height, args.seed, nullptr);
        check(st, "bt_render_device");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        const double delta = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        sum_delta += delta;
        buffer_samples += rc.samples * nn;                 // Buffer::inc_samples, mod.rs:199
        if (!args.stats_json.empty()) {
            bt_stats cs{};
            bt_scene_last_stats(scene, &cs);
            char row[256];
            std::snprintf(row, sizeof row, "%s{\"kernel_ms\": %.5f, \"segments\": %llu, \"samples\": %llu, \"pixels\": %llu, \"slices\": %u, \"packed\": %u}",
                          per_call.empty() ? "" : ", ", cs.kernel_ms, (unsigned long long)cs.segments,
                          (unsigned long long)cs.samples, (unsigned long long)cs.pixels, cs.slices, cs.packed);
            per_call += row;
        }
        if (!args.quiet)
            std::fprintf(stderr, "bendy tracer; samples: %u/%u; delta t: %s\n", buffer_samples, args.samples,
                         fmt_duration(delta / (rc.samples * nn)).c_str());
    }
    const double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
    bt_stats stats{};
    bt_scene_last_stats(scene, &stats);
    if (args.temporal)
        std::fprintf(stderr, "temporal: %ld frames, history length mean %.2f, min %.2f samples per pixel\n", args.frames, history_mean, history_min);
    std::fprintf(stderr, "bendy tracer; samples: %u/%u; avg t per sample: %s; total t: %s\n", buffer_samples, args.samples,
                 fmt_duration(buffer_samples ? sum_delta / buffer_samples : 0.0).c_str(), fmt_duration(total).c_str());
    if (args.adaptive)
        std::fprintf(stderr, "%.1f Msamples/s (adaptive passes: %llu pixel-samples in %u passes, %u..%u samples per tile)\n",
                     sum_delta > 0 ? (double)astats.pixel_samples / sum_delta / 1e6 : 0.0, (unsigned long long)astats.pixel_samples,
                     astats.passes, astats.min_count, astats.max_count);
    else
    std::fprintf(stderr, "%.1f Msamples/s (render calls only)\n",
                 sum_delta > 0 ? (double)n_px * buffer_samples / sum_delta / 1e6 : 0.0);

    std::string despeckle_json;
    if (despeckle) {
        // the resolved mean of --adaptive (n = 1: tiles hold different counts), else the sums of the whole render; under --temporal
        // every frame has passed already and the counts are the last frame's
        if (args.adaptive)
            check(bt_despeckle_device(despeckle, d_mean, 1, d_despeckled, args.width, args.height, &sp, nullptr), "bt_despeckle_device");
        else if (!args.temporal)
            check(bt_despeckle_device(despeckle, d_frame, buffer_samples ? buffer_samples : 1, d_despeckled, args.width, args.height, &sp,
                                      nullptr),
                  "bt_despeckle_device");
        check(bt_despeckle_poll(despeckle, &sstats), "bt_despeckle_poll");
        std::fprintf(stderr, "despeckle: ratio %g, rank %u, radius %u: %u of %u pixels pulled down, %u sanitised\n", sp.ratio, sp.rank, sp.radius,
                     sstats.flagged, sstats.pixels, sstats.sanitised);
        char sj[200];
        std::snprintf(sj, sizeof sj, ", \"despeckle\": {\"ratio\": %.9g, \"rank\": %u, \"radius\": %u, \"flagged\": %u, \"sanitised\": %u}", sp.ratio,
                      sp.rank, sp.radius, sstats.flagged, sstats.sanitised);
        despeckle_json = sj;
    }
    std::string resample_json;                             // filled once the frame has been resampled
    std::string upscale_json;                              // filled once the frame has been upscaled
    std::string compare_json;                              // filled once the frame has been compared
    auto write_stats = [&](const char *display_json) {
        FILE *f = std::fopen(args.stats_json.c_str(), "w");
        if (!f) die("cannot write " + args.stats_json);
        char ad[320] = "";
        if (args.adaptive)
            std::snprintf(ad, sizeof ad, ", \"adaptive\": {\"active_tiles\": %u, \"tiles\": %u, \"min_count\": %u, \"max_count\": %u, \"pixel_samples\": %llu, \"passes\": %u}",
                          astats.active_tiles, astats.tiles, astats.min_count, astats.max_count, (unsigned long long)astats.pixel_samples, astats.passes);
        if (args.temporal)
            std::snprintf(ad, sizeof ad, ", \"temporal\": {\"frames\": %ld, \"history_mean\": %.4f, \"history_min\": %.4f}", args.frames,
                          history_mean, history_min);
        std::fprintf(f, "{\"width\": %u, \"height\": %u, \"samples_per_call\": %u, \"subsample\": %u, \"calls\": [%s]%s%s%s}\n", args.width,
                     args.height, args.samples_per_call, args.subsample, per_call.c_str(), ad, (pick_json + despeckle_json + upscale_json + glare_json + resample_json + compare_json).c_str(), display_json);
        std::fclose(f);
    };
    // with the display or the resample stage: once the frame has been shown
    if (!args.stats_json.empty() && !display && !resample && !args.upscale) write_stats("");

    // Ctrl+P (main.rs:275-298)
    std::string shot = args.screenshot;
    if (!args.no_screenshot) {
        size_t slash = shot.find_last_of('/');
        std::string file = slash == std::string::npos ? shot : shot.substr(slash + 1);
        if (file.find('.') == std::string::npos)           // no extension -> with_file_name("render.png")
            shot = (slash == std::string::npos ? std::string() : shot.substr(0, slash + 1)) + "render.png";
        slash = shot.find_last_of('/');
        if (slash != std::string::npos && slash > 0) {
            std::string dir = shot.substr(0, slash);
            if (exists(dir)) {
                if (!is_dir(dir)) die(dir + " is not a directory");
            } else {
                create_dir_all(dir);
            }
        }
    }
    // --denoise (extension): the guides of the same frame into fresh buffers, then the screenshot shows the denoised mean
    float *d_shown = despeckle && !args.temporal ? d_despeckled : d_frame;
    unsigned shown_samples = buffer_samples ? buffer_samples : 1;
    if (args.temporal) {                                    // everything below sees the accumulated mean
        d_shown = d_mean;
        shown_samples = 1;
    }
    if (args.adaptive) {                                    // everything below sees the resolved mean
        d_shown = despeckle ? d_despeckled : d_mean;
        shown_samples = 1;
        if (!args.adaptive_map.empty()) {
            // the per-tile counts as a grey image, one pixel per tile, 255 = the cap
            std::vector<uint32_t> counts((size_t)astats.tiles);
            check(bt_adaptive_counts(adaptive, counts.data(), astats.tiles), "bt_adaptive_counts");
            const unsigned tx = (args.width + BT_TILE - 1) / BT_TILE, ty = (args.height + BT_TILE - 1) / BT_TILE;
            std::vector<uint8_t> grey((size_t)tx * ty * 4);
            for (size_t t = 0; t < counts.size(); ++t) {
                const uint8_t v = (uint8_t)std::min<uint64_t>(255, (uint64_t)counts[t] * 255 / std::max(1u, args.samples));
                grey[4 * t] = grey[4 * t + 1] = grey[4 * t + 2] = v;
                grey[4 * t + 3] = 255;
            }
            check(bt_write_png(args.adaptive_map.c_str(), grey.data(), tx, ty), "bt_write_png (--adaptive-map)");
            std::fprintf(stderr, "saved count map to %s\n", args.adaptive_map.c_str());
        }
    }
    if (args.denoise_inline && !args.no_screenshot) {
        bt_denoiser *dn = bt_denoiser_new();
        check(bt_denoise_device(dn, d_shown, shown_samples, d_guides[0], shown_samples, d_guides[1], shown_samples, d_guides[2],
                                shown_samples, d_guides[3], args.width, args.height, nullptr, nullptr),
              "bt_denoise_device");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        bt_denoiser_free(dn);
        d_shown = d_guides[3];
        shown_samples = 1;                                  // the denoised buffer holds a mean
        std::fprintf(stderr, "denoised with in-pass guides of %u samples\n", buffer_samples);
    }
    if (args.denoise && args.temporal && !args.no_screenshot) {      // the last frame's own guides, rendered with its colour
        const uint32_t gs = args.samples * nn;
        bt_denoiser *dn = bt_denoiser_new();
        check(bt_denoise_device(dn, d_shown, shown_samples, d_guides[0], gs, d_guides[1], gs, d_guides[2], gs, d_guides[3],
                                args.width, args.height, nullptr, nullptr),
              "bt_denoise_device");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        bt_denoiser_free(dn);
        d_shown = d_guides[3];
        std::fprintf(stderr, "denoised with the last frame's guides of %u samples\n", gs);
    }
    if (args.denoise && !args.temporal && !args.no_screenshot) {
        for (int g = 0; g < 4; ++g) {
            hip_check(hipMalloc((void **)&d_guides[g], n_px * 16), "hipMalloc");
            hip_check(hipMemcpy(d_guides[g], init.data(), n_px * 16, hipMemcpyHostToDevice), "hipMemcpy");
        }
        const int aov[3] = {BT_OUTPUT_ALBEDO, BT_OUTPUT_NORMAL, BT_OUTPUT_DEPTH};
        bt_config gcfg = cfg;
        bt_render_config grc = rc;
        grc.samples = args.denoise_guide_samples;
        grc.sample_base = 0;
        for (int g = 0; g < 3; ++g) {
            gcfg.output = aov[g];
            check(bt_render_device(scene, camera, &gcfg, &grc, d_guides[g], args.width, args.height, args.seed, nullptr),
                  "bt_render_device (denoise guide)");
        }
        const uint32_t gs = args.denoise_guide_samples * nn;
        bt_denoiser *dn = bt_denoiser_new();
        check(bt_denoise_device(dn, d_shown, shown_samples, d_guides[0], gs, d_guides[1], gs, d_guides[2], gs, d_guides[3],
                                args.width, args.height, nullptr, nullptr),
              "bt_denoise_device");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        bt_denoiser_free(dn);
        d_shown = d_guides[3];
        shown_samples = 1;                                  // the denoised buffer holds a mean
        std::fprintf(stderr, "denoised with guides of %u samples\n", gs);
    }
    // --upscale (extension): the three guides again at the shown size, first hit only, then the mean that is about to be shown
    // passes the upscale stage with the colour pass's own guides as the lo side
    bt_upscale *upscale = nullptr;
    float *d_hi[3] = {nullptr, nullptr, nullptr}, *d_upscaled = nullptr;
    if (args.upscale) {
        upscale = bt_upscale_new();
        if (!upscale) die(bt_last_error());
        std::vector<float> hi_init(n_shown * 4, 0.0f);
        for (size_t i = 0; i < n_shown; ++i) hi_init[4 * i + 3] = 1.0f;
        const int aov[3] = {BT_OUTPUT_ALBEDO, BT_OUTPUT_NORMAL, BT_OUTPUT_DEPTH};
        bt_config gcfg = cfg;
        bt_render_config grc = rc;
        grc.samples = args.upscale_guide_samples >= 0 ? (uint32_t)args.upscale_guide_samples : 1u;
        grc.sample_base = 0;
        for (int g = 0; g < 3; ++g) {
            hip_check(hipMalloc((void **)&d_hi[g], n_shown * 16), "hipMalloc");
            hip_check(hipMemcpy(d_hi[g], hi_init.data(), n_shown * 16, hipMemcpyHostToDevice), "hipMemcpy");
            gcfg.output = aov[g];
            check(bt_render_device(scene, camera, &gcfg, &grc, d_hi[g], shown_w, shown_h, args.seed, nullptr), "bt_render_device (upscale guide)");
        }
        hip_check(hipMalloc((void **)&d_upscaled, n_shown * 16), "hipMalloc");
        const uint32_t ls = buffer_samples ? buffer_samples : 1, hs = grc.samples * nn;
        const bt_upscale_guides lo = {d_guides[0], ls, d_guides[1], ls, d_guides[2], ls}, hi = {d_hi[0], hs, d_hi[1], hs, d_hi[2], hs};
        check(bt_upscale_device(upscale, d_shown, shown_samples, args.width, args.height, &lo, &hi, d_upscaled, shown_w, shown_h, nullptr, nullptr),
              "bt_upscale_device");
        bt_upscale_stats us{};
        check(bt_upscale_poll(upscale, &us), "bt_upscale_poll");
        d_shown = d_upscaled;
        shown_samples = 1;                                  // the upscaled buffer holds a mean
        std::fprintf(stderr, "upscale: %ux%u -> %ux%u with guides of %u samples: %u pixels took the 4 x 4 footprint, %u fell back to bilinear\n",
                     args.width, args.height, shown_w, shown_h, hs, us.tier2, us.tier3);
        char uj[160];
        std::snprintf(uj, sizeof uj, ", \"upscale\": {\"width\": %u, \"height\": %u, \"tier2\": %u, \"tier3\": %u}", shown_w, shown_h, us.tier2, us.tier3);
        upscale_json = uj;
        if (!args.stats_json.empty() && !display) write_stats("");
    }
    if (glare) {
        check(bt_glare_device(glare, d_shown, shown_samples, d_glare, glare_w, glare_h, &gp, nullptr), "bt_glare_device");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        d_shown = d_glare;
        shown_samples = 1;                                  // the glared buffer holds a mean
        std::fprintf(stderr, "glare: strength %g over %u levels, spread %g\n", gp.strength, glare_levels, gp.spread);
    }
    if (resample) {
        check(bt_resample_device(resample, d_shown, shown_samples, args.width, args.height, d_resampled, shown_w, shown_h, &rp, nullptr),
              "bt_resample_device");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        d_shown = d_resampled;
        shown_samples = 1;                                  // the resampled buffer holds a mean
        const int taps_x = bt_debug_resample_weights(resample, 0, nullptr, nullptr, nullptr, nullptr);
        const int taps_y = bt_debug_resample_weights(resample, 1, nullptr, nullptr, nullptr, nullptr);
        check(std::min(taps_x, taps_y), "bt_debug_resample_weights");
        const char *names[4] = {"box", "tent", "mitchell", "lanczos3"};
        std::fprintf(stderr, "resample: %ux%u -> %ux%u, %s, %d x %d taps\n", args.width, args.height, shown_w, shown_h, names[rp.filter], taps_x,
                     taps_y);
        char rj[192];
        std::snprintf(rj, sizeof rj, ", \"resample\": {\"width\": %u, \"height\": %u, \"filter\": \"%s\", \"taps_x\": %d, \"taps_y\": %d}", shown_w,
                      shown_h, names[rp.filter], taps_x, taps_y);
        resample_json = rj;
        if (!args.stats_json.empty() && !display) write_stats("");
    }
    // --compare (extension): the frame --hdr would write against the truth; nothing below reads what this writes
    if (!args.compare.empty()) {
        std::vector<float> truth(n_shown * 4);
        uint32_t tw = 0, th = 0;
        check(bt_read_pfm(args.compare.c_str(), truth.data(), truth.size(), &tw, &th), "bt_read_pfm");
        if (tw != shown_w || th != shown_h) die("--compare: " + args.compare + " changed its size");
        float *d_truth = nullptr;
        hip_check(hipMalloc((void **)&d_truth, n_shown * 16), "hipMalloc");
        hip_check(hipMemcpy(d_truth, truth.data(), n_shown * 16, hipMemcpyHostToDevice), "hipMemcpy");
        bt_compare *cmp = bt_compare_new();
        if (!cmp) die(bt_last_error());
        bt_compare_params cp;
        bt_compare_params_default(&cp);
        bt_compare_stats cs{};
        check(bt_compare_device(cmp, d_shown, shown_samples, d_truth, 1, shown_w, shown_h, &cp, nullptr), "bt_compare_device");
        check(bt_compare_poll(cmp, &cs), "bt_compare_poll");
        const double fraction = args.compare_tail >= 0.0 ? args.compare_tail : 0.01;
        double share = 0.0;
        check(bt_compare_tail(cmp, fraction, &share, nullptr), "bt_compare_tail");
        const unsigned long long max_x = cs.max_index % shown_w, max_y = cs.max_index / shown_w;
        char psnr[40];
        if (std::isfinite(cs.psnr)) std::snprintf(psnr, sizeof psnr, "%.17g", cs.psnr);
        else std::snprintf(psnr, sizeof psnr, "null");
        if (!args.quiet)
            std::fprintf(stderr, "compare: against %s: MSE %.6g, relMSE %.6g, PSNR %s dB, SSIM %.6f, max |d| %.6g at (%llu, %llu), %llu valid and %llu "
                         "non-finite pixels, the worst %g of them carry %.4f of the error\n", args.compare.c_str(), cs.mse, cs.rel_mse,
                         std::isfinite(cs.psnr) ? psnr : "inf", cs.ssim, cs.max_abs, max_x, max_y, (unsigned long long)cs.valid,
                         (unsigned long long)cs.nonfinite, fraction, share);
        char cj[640];
        std::snprintf(cj, sizeof cj, ", \"compare\": {\"mse\": %.17g, \"rel_mse\": %.17g, \"psnr\": %s, \"ssim\": %.17g, \"max_abs\": %.17g, \"max_x\": %llu, "
                      "\"max_y\": %llu, \"valid\": %llu, \"nonfinite\": %llu, \"tail_fraction\": %.17g, \"tail_share\": %.17g}", cs.mse, cs.rel_mse, psnr,
                      cs.ssim, cs.max_abs, max_x, max_y, (unsigned long long)cs.valid, (unsigned long long)cs.nonfinite, fraction, share);
        compare_json = cj;
        if (!args.compare_map.empty()) {
            uint8_t *d_map = nullptr;
            hip_check(hipMalloc((void **)&d_map, n_shown * 4), "hipMalloc");
            check(bt_compare_map_device(cmp, d_map, args.compare_map_scale >= 0.0f ? args.compare_map_scale : 1.0f, nullptr), "bt_compare_map_device");
            std::vector<uint8_t> map8(n_shown * 4);
            hip_check(hipMemcpy(map8.data(), d_map, n_shown * 4, hipMemcpyDeviceToHost), "hipMemcpy");
            check(bt_write_png(args.compare_map.c_str(), map8.data(), shown_w, shown_h), "bt_write_png (--compare-map)");
            if (!args.quiet) std::fprintf(stderr, "saved error map to %s\n", args.compare_map.c_str());
            (void)hipFree(d_map);
        }
        bt_compare_free(cmp);
        (void)hipFree(d_truth);
        if (!args.stats_json.empty() && !display) write_stats("");
    }
    if (display) {
        check(bt_display_device(display, d_shown, shown_samples, d_rgba8, shown_w, shown_h, color_space, &dp, nullptr), "bt_display_device");
        float ev = 0.0f, mult = 0.0f;
        uint32_t counters[258];
        check(bt_display_exposure(display, &ev, &mult), "bt_display_exposure");
        check(bt_debug_display_histogram(display, counters, 258), "bt_debug_display_histogram");
        std::fprintf(stderr, "display: %s, exposure %s %+.4f EV (x %.5f), %u pixels under, %u over the metered range\n", args.tonemap.c_str(),
                     args.exposure_auto ? "auto" : "manual", ev, mult, counters[256], counters[257]);
        if (!args.stats_json.empty()) {
            char dj[256];
            std::snprintf(dj, sizeof dj, ", \"display\": {\"ev\": %.9g, \"mult\": %.9g, \"under\": %u, \"over\": %u, \"operator\": \"%s\"}", ev, mult,
                          counters[256], counters[257], args.tonemap.c_str());
            write_stats(dj);
        }
    }
    if (!args.hdr.empty()) {
        std::vector<float> lin(n_shown * 4);
        hip_check(hipMemcpy(lin.data(), d_shown, n_shown * 16, hipMemcpyDeviceToHost), "hipMemcpy");
        check(bt_write_pfm(args.hdr.c_str(), lin.data(), shown_w, shown_h, shown_samples), "bt_write_pfm");
        std::fprintf(stderr, "saved linear frame to %s\n", args.hdr.c_str());
    }
    if (!args.no_screenshot) {
        if (!display)
            check(bt_preview_device(d_shown, d_rgba8, shown_w, shown_h, shown_samples, color_space, nullptr),
                  "bt_preview_device");
        std::vector<uint8_t> rgba8(n_shown * 4);
        hip_check(hipMemcpy(rgba8.data(), d_rgba8, n_shown * 4, hipMemcpyDeviceToHost), "hipMemcpy");
        check(bt_write_png(shot.c_str(), rgba8.data(), shown_w, shown_h), "bt_write_png");
        std::fprintf(stderr, "saved screenshot to %s\n", shot.c_str());
    }

    // Ctrl+K (main.rs:299-313)
    if (!args.save_scene.empty()) {
        check(bt_scene_save(scene, args.save_scene.c_str()), "bt_scene_save");
        std::fprintf(stderr, "saved scene to %s\n", args.save_scene.c_str());
    }

    (void)hipFree(d_frame);
    (void)hipFree(d_rgba8);
    if (d_mean) (void)hipFree(d_mean);
    bt_adaptive_free(adaptive);
    bt_temporal_free(temporal);
    bt_display_free(display);
    bt_despeckle_free(despeckle);
    if (d_despeckled) (void)hipFree(d_despeckled);
    bt_glare_free(glare);
    if (d_glare) (void)hipFree(d_glare);
    bt_resample_free(resample);
    if (d_resampled) (void)hipFree(d_resampled);
    bt_upscale_free(upscale);
    if (d_upscaled) (void)hipFree(d_upscaled);
    for (float *g : d_hi)
        if (g) (void)hipFree(g);
    for (float *g : d_guides)
        if (g) (void)hipFree(g);
    bt_scene_free(scene);
    return 0;
}
