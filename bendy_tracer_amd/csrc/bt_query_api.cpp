// bt_query_api.cpp -- EXTENSION, NOT IN THE REFERENCE: the C ABI of the ray query API (include/bendy_hip.h, bt_query_rays_device
// and its neighbours).  Validation and the launches; the kernels are in bt_query.hip, the scene's tables come from
// bt_api.cpp through bt_scene_query_tables_internal.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/bendy_hip.h"
#include "bt_internal.hpp"
#include "bt_view.hpp"

#pragma STDC FP_CONTRACT OFF

namespace {

bool misaligned(const void *p) { return ((uintptr_t)p & 15u) != 0; }

// frees a device allocation when the scope is left
struct DeviceBytes {
    void *ptr = nullptr;
    ~DeviceBytes() {
        if (ptr) (void)hipFree(ptr);
    }
};

} // namespace

extern "C" {

int bt_query_rays_device(bt_scene *scene, const bt_ray *rays_device, uint32_t n, bt_hit *hits_device, void *stream) {
    // in the order the header gives
    if (!scene || !rays_device || !hits_device) return fail(BT_ERR_INVALID_ARG, "null scene, rays or hits");
    if (misaligned(rays_device) || misaligned(hits_device) || (const void *)rays_device == (const void *)hits_device)
        return fail(BT_ERR_INVALID_ARG, "rays and hits must be 16-byte aligned and two buffers");
    if (n >= (1u << 30)) return fail(BT_ERR_INVALID_ARG, "a query takes fewer than 2^30 rays");
    if (bt_scene_lens_on_internal(scene)) return fail(BT_ERR_UNSUPPORTED, "queries are straight rays: the lens extension has none");
    if (n == 0) return 0;
    BtQueryLaunch Q{};
    int rc = bt_scene_query_tables_internal(scene, &Q.prims, &Q.refs, &Q.n_prims);   // BT_ERR_DEVICE without a device
    if (rc) return rc;
    Q.rays = rays_device;
    Q.hits = hits_device;
    Q.n = n;
    BT_HIP(bt_launch_query(&Q, (hipStream_t)stream));
    return (int)n;
}

int bt_view_rays_device(const bt_view *view, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, bt_ray *rays_device, void *stream) {
    if (!view || !rays_device || misaligned(rays_device)) return fail(BT_ERR_INVALID_ARG, "null view, or rays null or not 16-byte aligned");
    BtViewRaysLaunch P{};
    if (!btview::prepare(*view, P.view)) return fail(BT_ERR_INVALID_ARG, "a view with a non-finite entry, an empty frustum, clip range or frame, or a singular matrix");
    if (w == 0 || h == 0) return fail(BT_ERR_INVALID_ARG, "an empty rectangle");
    if (x0 >= view->width || w > view->width - x0 || y0 >= view->height || h > view->height - y0)
        return fail(BT_ERR_INVALID_ARG, "the rectangle leaves the " + std::to_string(view->width) + " x " + std::to_string(view->height) + " frame");
    if ((uint64_t)w * h >= (1ull << 30)) return fail(BT_ERR_INVALID_ARG, "a rectangle of 2^30 pixels and more");
    int dev = -1;
    BT_HIP(hipGetDevice(&dev));          // BT_ERR_DEVICE without a device
    P.x0 = x0; P.y0 = y0; P.w = w; P.h = h;
    P.rays = rays_device;
    BT_HIP(bt_launch_view_rays(&P, (hipStream_t)stream));
    return (int)(w * h);
}

int bt_scene_pick(bt_scene *scene, uint64_t camera_ref, const bt_config *config, const bt_render_config *render, uint32_t width,
                  uint32_t height, uint32_t x, uint32_t y, bt_hit *hit, float *focus) {
    if (!hit) return fail(BT_ERR_INVALID_ARG, "null hit");
    bt_view view;
    int rc = bt_scene_camera_view(scene, camera_ref, config, render, width, height, &view);
    if (rc) return rc;
    if (x >= width || y >= height)
        return fail(BT_ERR_INVALID_ARG, "pixel (" + std::to_string(x) + ", " + std::to_string(y) + ") is outside the " + std::to_string(width) + " x " + std::to_string(height) + " frame");
    if (bt_scene_lens_on_internal(scene)) return fail(BT_ERR_UNSUPPORTED, "queries are straight rays: the lens extension has none");
    btview::View V;
    if (!btview::prepare(view, V)) return fail(BT_ERR_INVALID_ARG, "a view with a non-finite entry, an empty frustum, clip range or frame, or a singular matrix");
    int dev = -1;
    BT_HIP(hipGetDevice(&dev));
    DeviceBytes d;                       // one ray, then one hit: 96 B
    BT_HIP(hipMalloc(&d.ptr, sizeof(bt_ray) + sizeof(bt_hit)));
    bt_ray *d_ray = (bt_ray *)d.ptr;
    bt_hit *d_hit = (bt_hit *)((char *)d.ptr + sizeof(bt_ray));
    rc = bt_view_rays_device(&view, x, y, 1, 1, d_ray, nullptr);
    if (rc < 0) return rc;
    rc = bt_query_rays_device(scene, d_ray, 1, d_hit, nullptr);
    if (rc < 0) return rc;
    BT_HIP(hipMemcpy(hit, d_hit, sizeof(bt_hit), hipMemcpyDeviceToHost));   // behind both kernels on the null stream; blocks the host
    if (hit->face < 0) return 0;
    if (focus) *focus = btview::focus_of(V, (float)x, (float)y, hit->t);
    return 1;
}

} // extern "C"
