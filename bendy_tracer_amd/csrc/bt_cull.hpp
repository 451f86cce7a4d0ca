// bt_cull.hpp -- which spheres the primary rays of a pixel block can reach.
//
// Used by the sphere-only build without volumes (bt_kernels.hip: a block whose mask is empty traces nothing) and, for
// tests, on the host (bt_debug_primary_mask).  Bit i of a block's mask is CLEAR only when it is proven that no camera
// ray of the block (bt_kernels.hip, the camera event) makes sphere row i pass intersect_spheres_plain's `ok` test.
// Everything here is double precision with margins far above the float kernel's rounding; the derivation is in
// DESIGN.md 5.15, the short form next to the code.
#pragma once
#include <stdint.h>

#include "bt_types.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define BT_HD __host__ __device__ inline
#else
#define BT_HD inline
#endif

namespace btcull {

struct D3 { double x, y, z; };
BT_HD D3 d3(double x, double y, double z) { D3 r; r.x = x; r.y = y; r.z = z; return r; }
BT_HD D3 d3(const BtV3 &a) { return d3((double)a.x, (double)a.y, (double)a.z); }
BT_HD D3 sub(D3 a, D3 b) { return d3(a.x - b.x, a.y - b.y, a.z - b.z); }
BT_HD double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
BT_HD D3 dcross(D3 a, D3 b) { return d3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
BT_HD double dabs(double v) { return v < 0.0 ? -v : v; }
BT_HD double dmin(double a, double b) { return a < b ? a : b; }
BT_HD double dmax(double a, double b) { return a > b ? a : b; }
BT_HD double dsqrt(double v) { return __builtin_sqrt(v); }
// sin / cos by their Taylor polynomials (the same operations on host and device, no libm), with a bound on what the
// polynomial leaves out: |x|^11 / 11! and |x|^12 / 12!
BT_HD void taylor_sincos(double x, double &s, double &c, double &err) {
    const double x2 = x * x;
    s = x * (1.0 + x2 * (-1.0 / 6.0 + x2 * (1.0 / 120.0 + x2 * (-1.0 / 5040.0 + x2 * (1.0 / 362880.0)))));
    c = 1.0 + x2 * (-0.5 + x2 * (1.0 / 24.0 + x2 * (-1.0 / 720.0 + x2 * (1.0 / 40320.0 + x2 * (-1.0 / 3628800.0)))));
    const double x4 = x2 * x2, x11 = x4 * x4 * x2 * dabs(x);
    err = x11 * (1.0 / 39916800.0) + x11 * dabs(x) * (1.0 / 479001600.0) + 1e-15;
}

// The block's primary rays, bounded: every one starts within `rho` of `apex` and runs, for t >= 0, in a direction
// within the angle asin(sin_a) of the unit axis `axis`.  ok = 0: nothing could be bounded, every sphere stays in.
struct Cone {
    D3 apex, axis;
    double sin_a, cos_a, rho;
    int ok;
};

// Pixels [px0, px0 + nx) x [py0, py0 + ny) of a launch (nx, ny >= 1).
BT_HD Cone primary_cone(const BtLaunch &P, uint32_t px0, uint32_t py0, uint32_t nx, uint32_t ny) {
    Cone K;
    K.ok = 0;
    K.apex = d3(P.cam_t);
    K.axis = d3(0.0, 0.0, 0.0);
    K.sin_a = 1.0; K.cos_a = 0.0; K.rho = 0.0;
    // a negative / NaN clip_min would let roots behind the origin count; the camera's columns must be a rotation times a
    // scale (angles between directions kept); otherwise no bound
    if (!((double)P.clip_min >= 0.0)) return K;
    const D3 mx = d3(P.cam_cx), my = d3(P.cam_cy), mz = d3(P.cam_cz);
    const double g00 = ddot(mx, mx), g11 = ddot(my, my), g22 = ddot(mz, mz);
    const double s2 = (g00 + g11 + g22) * (1.0 / 3.0);
    if (!(s2 >= 1e-30 && s2 <= 1e30)) return K;
    const double tol = 1e-5 * s2;
    if (!(dabs(g00 - s2) <= tol && dabs(g11 - s2) <= tol && dabs(g22 - s2) <= tol && dabs(ddot(mx, my)) <= tol &&
          dabs(ddot(mx, mz)) <= tol && dabs(ddot(my, mz)) <= tol))
        return K;
    const double s = dsqrt(s2);

    // uu = (px * pixel_width - 1) + (u_sub * pixel_width + jitter): each term's range, added up (likewise vv)
    const double n = (double)(P.subsample_n > 1 ? P.subsample_n : 1);
    const double sub_hi = (n - 1.0) / n;
    const double pw = (double)P.pixel_width, ph = (double)P.pixel_height;
    const double ju0 = (double)P.jitter_u_lo, ju1 = ju0 + (double)P.jitter_u_scale;
    const double jv0 = (double)P.jitter_v_lo, jv1 = jv0 + (double)P.jitter_v_scale;
    const double ua = (double)px0 * pw - 1.0, ub = (double)(px0 + nx - 1u) * pw - 1.0;
    const double va = (double)py0 * ph - 1.0, vb = (double)(py0 + ny - 1u) * ph - 1.0;
    const double uu_lo = dmin(ua, ub) + dmin(0.0, sub_hi * pw) + dmin(ju0, ju1);
    const double uu_hi = dmax(ua, ub) + dmax(0.0, sub_hi * pw) + dmax(ju0, ju1);
    const double vv_lo = dmin(va, vb) + dmin(0.0, sub_hi * ph) + dmin(jv0, jv1);
    const double vv_hi = dmax(va, vb) + dmax(0.0, sub_hi * ph) + dmax(jv0, jv1);
    // yrot = xfov / 2 * -uu, xrot = yfov / 2 * -vv; widened by far more than the float evaluation's error (~1e-6 rad)
    const double hxf = 0.5 * (double)P.xfov, hyf = 0.5 * (double)P.yfov;
    const double wid = 1e-5 * (1.0 + dabs(hxf) + dabs(hyf));
    const double y_lo = dmin(-hxf * uu_lo, -hxf * uu_hi) - wid, y_hi = dmax(-hxf * uu_lo, -hxf * uu_hi) + wid;
    const double x_lo = dmin(-hyf * vv_lo, -hyf * vv_hi) - wid, x_hi = dmax(-hyf * vv_lo, -hyf * vv_hi) + wid;
    const double ym = 0.5 * (y_lo + y_hi), xm = 0.5 * (x_lo + x_hi);
    if (!(dabs(ym) <= 1.6 && dabs(xm) <= 1.6)) return K;
    // d_cam(yrot, xrot) = (-cos x sin y, sin x, -cos x cos y) has |dd|^2 = cos^2 x dy^2 + dx^2 <= dy^2 + dx^2: every
    // direction of the rectangle lies within half its diagonal (an angle) of the centre's direction
    const double hy = 0.5 * (y_hi - y_lo), hx = 0.5 * (x_hi - x_lo);
    double alpha = dsqrt(hy * hy + hx * hx);
    double sy, cy, ey, sx, cx, ex;
    taylor_sincos(ym, sy, cy, ey);
    taylor_sincos(xm, sx, cx, ex);
    alpha += 8.0 * (ey + ex);                      // the centre direction's polynomial error, as an angle
    const D3 dc = d3(-(cx * sy), sx, -(cx * cy));
    D3 ax = d3((mx.x * dc.x + my.x * dc.y) + mz.x * dc.z, (mx.y * dc.x + my.y * dc.y) + mz.y * dc.z,
               (mx.z * dc.x + my.z * dc.y) + mz.z * dc.z);
    const double al = dsqrt(ddot(ax, ax));
    if (!(al > 0.0)) return K;
    ax = d3(ax.x / al, ax.y / al, ax.z / al);
    // the kernel's float rounding of the direction (sin / cos, transform, normalisations: ~1e-6 rad) and the camera
    // matrix's distance from a scaled rotation (<= 1e-5 relative): both well inside 2e-4 rad
    alpha += 2e-4;
    double rho = 0.0;
    if (P.has_focus) {
        // origin cam_t + M (aperture (disk_x cs + disk_y sn) r2) with r2 <= one_scale and cs^2 + sn^2 <= 1 + 1e-6:
        // |disk_x cs + disk_y sn|^2 <= (cs^2 + sn^2) lmax, lmax <= max(|disk_x|^2, |disk_y|^2) + |disk_x . disk_y| the
        // larger eigenvalue of their Gram matrix (orthonormal disk_x, disk_y: lmax = 1).  The 1e-4 covers that 1e-6, the
        // float products and the matrix's 1e-5.  Direction f d1 - offset with f = focus / |d_cam.z| >= focus: it leans
        // away from d1 by at most asin(rho / focus) <= r + r^3 (r <= 1/2)
        const D3 dx = d3(P.disk_x), dy = d3(P.disk_y);
        const double lmax = dmax(ddot(dx, dx), ddot(dy, dy)) + dabs(ddot(dx, dy));
        rho = s * dabs((double)P.aperture) * dsqrt(lmax) * dabs((double)P.one_scale) * (1.0 + 1e-4);
        const double f_lo = (double)P.focus * (1.0 - 1e-5);
        if (!(f_lo > 0.0)) return K;
        const double r = rho / f_lo;
        if (!(r <= 0.5)) return K;
        alpha += r + r * r * r;
    }
    // the float origin: cam_t + offset rounded
    rho += 1e-6 * (dabs(K.apex.x) + dabs(K.apex.y) + dabs(K.apex.z)) + 1e-30;
    // alpha bounds the true angle; asin(alpha) >= alpha, so (sin, cos) = (alpha, sqrt(1 - alpha^2)) is a wider cone
    if (!(alpha <= 0.9)) return K;
    K.axis = ax;
    K.sin_a = alpha;
    K.cos_a = dsqrt(1.0 - alpha * alpha);
    K.rho = rho;
    K.ok = 1;
    return K;
}

// May a ray of the cone pass intersect_spheres_plain's test for the sphere row (c, r2)?  The kernel's float disc =
// half_b^2 - cc is within 14 eps (|oc|^2 + r2) of the exact value, and |d|^2 within 1e-6 of 1: a ray whose line passes
// farther than R = sqrt(r2 + 2^-12 (|oc|^2 + r2)) from c has disc < 0, and one whose half-line t >= 0 stays farther
// than R has no root >= clip_min >= 0.  The half-lines lie within rho of the cone from the apex.
BT_HD bool may_hit(const Cone &K, float cx, float cy, float cz, float r2) {
    if (!K.ok) return true;
    const D3 v = sub(d3((double)cx, (double)cy, (double)cz), K.apex);
    const double D = dsqrt(ddot(v, v));
    const double lam = D + K.rho;
    const double R = dsqrt((double)r2 + 0x1p-12 * (lam * lam + (double)r2));
    const double va = ddot(v, K.axis);
    const D3 cr = dcross(v, K.axis);
    const double vc = dsqrt(ddot(cr, cr));
    // distance from c to the cone: D when the angle between v and the axis exceeds alpha + pi/2 (the apex is nearest),
    // 0 inside it, else D sin(angle - alpha)
    const double cos_part = va * K.cos_a + vc * K.sin_a, sin_part = vc * K.cos_a - va * K.sin_a;
    const double dist = cos_part <= 0.0 ? D : (sin_part <= 0.0 ? 0.0 : sin_part);
    return !(dist > R + K.rho);
}

} // namespace btcull
