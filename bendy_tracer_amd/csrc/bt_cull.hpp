// bt_cull.hpp -- which spheres the primary rays of a pixel block can reach.
//
// Used for the sphere-only build without volumes: bt_block_mask_kernel (bt_kernels.hip) writes one 64-bit mask per pixel
// block of a launch, the render kernel reads its block's mask and traces nothing when it is empty.  The same function,
// block_mask(), runs on the host for tests (bt_debug_primary_mask).  Bit i of a block's mask is CLEAR only when it is
// proven that no camera ray of the block (bt_kernels.hip, the camera event) makes sphere row i pass
// intersect_spheres_plain's `ok` test.
// Everything here is double precision with margins far above the float kernel's rounding; the derivation is in
// DESIGN.md 5.15, the short form next to the code.
#pragma once
#include <stdint.h>
#include <string.h>

#include "bt_types.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define BT_HD __host__ __device__ inline
#define BT_HDF static __host__ __device__ __forceinline__
#else
#define BT_HD inline
#define BT_HDF static inline
#endif

// ---- where a pixel block lies in the frame ---------------------------------------------------------------------------
// BtLaunch::slices = NS in {1,2,4,8,16,32}: a 16x16 tile is cut into NS blocks of pxb = 256/NS pixels -- whole 8x8 quadrants
// down to 64 pixels, then 8x4, 4x4, 4x2 pixels, numbered row-major inside the tile.  Block b of the launch is block
// b mod NS of the launch's tile b / NS.  The tile (a division by tiles_x: umulhi + one fix-up step) and the block's corner
// inside it depend on the block alone: computed once per block (wave-uniform: scalar), not once per work item.
struct BlockGeom { uint32_t NS, LOG_NS, pxb, LOG_PXB, LBW, WMASK; };
BT_HDF BlockGeom block_geom(const BtLaunch &P) {
    BlockGeom g;
    g.NS = (uint32_t)P.slices;
    g.LOG_NS = (uint32_t)__builtin_ctz(g.NS);
    g.pxb = 256u >> g.LOG_NS;                          // pixels per block
    g.LOG_PXB = 8u - g.LOG_NS;
    g.LBW = g.pxb >= 32 ? 3u : 2u;                     // log2 of a block row: whole quadrants and 8x4 blocks are 8 pixels wide
    g.WMASK = (1u << g.LBW) - 1u;
    return g;
}
struct BlockRef { uint32_t px0, py0, tile_ok, slot; };
BT_HDF BlockRef block_ref(const BtLaunch &P, const BlockGeom &g, uint32_t b) {      // b: block in launch order
    const uint32_t slot = b >> g.LOG_NS, sub = b & (g.NS - 1u);
    const uint32_t tile = P.sharded ? (slot * P.world + P.rank) : slot;
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t ty = __umulhi(tile, P.tiles_x_magic), tx = tile - ty * P.tiles_x;      // tile / tiles_x, exact after the fix-up
#else
    uint32_t ty = (uint32_t)(((uint64_t)tile * P.tiles_x_magic) >> 32), tx = tile - ty * P.tiles_x;
#endif
    if (tx >= P.tiles_x) { ty += 1u; tx -= P.tiles_x; }
    // corner of block `sub` inside the tile: 128 pixels = the quadrant row `sub`, 64 = quadrant `sub`, below that blocks
    // of 8x4 / 4x4 / 4x2 pixels numbered row-major
    uint32_t bx0 = 0, by0 = 0;
    if (g.pxb == 128) by0 = sub << 3;
    else if (g.pxb == 64) { bx0 = (sub & 1u) << 3; by0 = (sub >> 1) << 3; }
    else if (g.pxb < 64) {
        const uint32_t lbh = g.LOG_PXB - g.LBW, lnbx = 4u - g.LBW;
        bx0 = (sub & ((1u << lnbx) - 1u)) << g.LBW;
        by0 = (sub >> lnbx) << lbh;
    }
    BlockRef r;
    r.px0 = tx * BT_TILE_DIM + bx0;
    r.py0 = ty * BT_TILE_DIM + by0;
    r.tile_ok = ty < P.tiles_y ? 1u : 0u;
    r.slot = slot;
    return r;
}
// the block's pixels inside the frame: the rectangle [px0, px0 + nx) x [py0, py0 + ny) (nx = 0 or ny = 0: none).  A block is
// 16 pixels wide when it holds whole rows of quadrants (pxb >= 128), else 2^LBW; pxb >> log2(width) rows high.
BT_HDF void block_extent(const BtLaunch &P, const BlockGeom &g, const BlockRef &B, uint32_t &nx, uint32_t &ny) {
    const uint32_t lw = g.pxb >= 128 ? 4u : g.LBW, bw = 1u << lw, bh = g.pxb >> lw;
    nx = B.tile_ok && B.px0 < P.width ? (P.width - B.px0 < bw ? P.width - B.px0 : bw) : 0u;
    ny = B.tile_ok && B.py0 < P.height ? (P.height - B.py0 < bh ? P.height - B.py0 : bh) : 0u;
}

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
    // The depth slices (a camera with focus; hg = 1).  In the camera's frame (rx, ry, rz: its unit axes in world space;
    // depth z along -rz, lateral = the (rx, ry) components), with beta = (d.x, d.y) / |d.z| of a camera-space direction d:
    // the ray through the lens point `off` (|off| <= rho, depth 0) and the focus point f * (beta, 1) is, at depth z,
    // at the lateral position off (1 - z / f) + z beta.  Every beta of the block lies within hg_w of (hg_bx, hg_by): at
    // depth z >= 0 the block's rays lie within rho |1 - z / f| + hg_w z of z * (hg_bx, hg_by) -- an hourglass with its
    // waist at the focus distance, two convex pieces [0, f] and [f, inf) whose radius is linear in z.
    int hg;
    D3 rx, ry, rz;
    double hg_bx, hg_by, hg_w, hg_f;
};

// Pixels [px0, px0 + nx) x [py0, py0 + ny) of a launch (nx, ny >= 1).
BT_HD Cone primary_cone(const BtLaunch &P, uint32_t px0, uint32_t py0, uint32_t nx, uint32_t ny) {
    Cone K;
    K.ok = 0;
    K.apex = d3(P.cam_t);
    K.axis = d3(0.0, 0.0, 0.0);
    K.sin_a = 1.0; K.cos_a = 0.0; K.rho = 0.0;
    K.hg = 0;
    K.rx = K.ry = K.rz = d3(0.0, 0.0, 0.0);
    K.hg_bx = K.hg_by = K.hg_w = K.hg_f = 0.0;
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
    const double alpha_dir = alpha;                // the block's directions d1 alone, before the lens leans them
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
    // The depth slices.  Every direction of the block lies within a_h of dc (alpha_dir, + 1e-4 for the camera frame: the
    // matrix is within ~2e-5 of s * rotation).  Directions at the angles th_c and th <= th_c + a_h from the camera's -z
    // axis, an angle g <= a_h apart, meet the plane z = -1 in points P, Q with |P| = 1 / cos th_c, |Q| = 1 / cos th; the
    // triangle (0, P, Q) has the area |P| |Q| sin g / 2 = |P - Q| h / 2 with h >= 1 the origin's distance from the line
    // P Q (which lies in the plane): |beta - beta_c| = |P - Q| <= sin a_h / (cos th_c cos(th_c + a_h)).
    // Only with disk_x, disk_y exactly in the lens plane (what fill_launch makes them).
#ifdef BT_NO_DEPTH_SLICES                          // A/B variant (make variant): the cone alone
    if (false) {
#else
    if (P.has_focus && (double)P.disk_x.z == 0.0 && (double)P.disk_y.z == 0.0) {
#endif
        const double a_h = alpha_dir + 1e-4;
        const double dl = dsqrt(ddot(dc, dc));
        if (dl > 0.5 && dl < 2.0) {
            const double cth = dabs(dc.z) / dl;
            const double sth = dsqrt(dmax(0.0, 1.0 - cth * cth)) + 1e-12;
            const double den = cth * (1.0 - 0.5 * a_h * a_h) - sth * a_h;          // <= cos(th_c + a_h)
            if (cth >= 0.1 && den >= 0.05 && dc.z < 0.0) {
                K.hg_w = a_h / (cth * den) * (1.0 + 1e-9);
                K.hg_bx = dc.x / dabs(dc.z);
                K.hg_by = dc.y / dabs(dc.z);
                K.hg_f = (double)P.focus;
                K.rx = d3(mx.x / s, mx.y / s, mx.z / s);
                K.ry = d3(my.x / s, my.y / s, my.z / s);
                K.rz = d3(mz.x / s, mz.y / s, mz.z / s);
                K.hg = 1;
            }
        }
    }
    return K;
}

// Does a tangent plane of the piece {z0 <= z <= z1, |lat - z beta_c| <= a + b z} separate it from the ball of radius R
// around (lat, z) = ((lx, ly), zc)?  With n the unit direction of l' = lat - zc beta_c, every point of the piece satisfies
// n . (lat - z beta_c) <= a + b z, i.e. N . p <= a for N = (n, -(beta_c . n + b)); the ball lies beyond that plane when
// N . c - a = |l'| - b zc - a > R |N|.  (z1 < 0: no upper end.)
BT_HD bool piece_separated(const Cone &K, double a, double b, double z0, double z1, double lx, double ly, double zc, double R) {
    if (zc + R < z0) return true;
    if (z1 >= 0.0 && zc - R > z1) return true;
    const double px = lx - zc * K.hg_bx, py = ly - zc * K.hg_by;
    const double pl = dsqrt(px * px + py * py);
    if (!(pl > 0.0)) return false;
    const double nz = (K.hg_bx * px + K.hg_by * py) / pl + b;
    const double nl = dsqrt(1.0 + nz * nz) * (1.0 + 1e-12);
    return pl - b * zc - a > R * nl;
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
    if (dist > R + K.rho) return false;
    if (!K.hg) return true;
    // The depth slices.  A float ray that passes the test comes within R of c at a distance t <= D + rho + R from its
    // origin; it leaves the exact ray of the same sample by at most 2e-4 t (direction after the lens: ~1e-6 rad of float
    // rounding; the camera frame against the matrix: ~2e-5 of every length) plus the origin's rounding (in K.rho).  So an
    // exact ray, which lies in the hourglass, comes within Rm of c: no hit when planes separate the ball from both pieces.
    const double Rm = R + 2e-4 * (D + K.rho + R) + 1e-6 * (dabs(K.apex.x) + dabs(K.apex.y) + dabs(K.apex.z)) + 1e-30;
    const double lx = ddot(v, K.rx), ly = ddot(v, K.ry), zc = -ddot(v, K.rz);
    const double f = K.hg_f, rl = K.rho;
    if (!piece_separated(K, rl, K.hg_w - rl / f, 0.0, f, lx, ly, zc, Rm)) return true;
    if (!piece_separated(K, -rl, K.hg_w + rl / f, f, -1.0, lx, ly, zc, Rm)) return true;
    return false;
}

// The mask of block `b` (launch order) of the launch `P`: bit i set = sphere row i may be hit by a primary ray of the
// block.  0 for a block without pixels in the frame and for an empty scene; every bit for a table of more than 64 rows.
// `rows` = the launch's BtSphereRow table (a host pointer, or the device table through the constant address space).
template <class Rows> BT_HD uint64_t block_mask(const BtLaunch &P, Rows rows, uint32_t b) {
    const BlockGeom G = block_geom(P);
    const BlockRef B = block_ref(P, G, b);
    uint32_t nx = 0, ny = 0;
    block_extent(P, G, B, nx, ny);
    if (nx == 0u || ny == 0u || P.n_prims <= 0) return 0ull;
    if (P.n_prims > 64) return ~0ull;
    const Cone K = primary_cone(P, B.px0, B.py0, nx, ny);
    uint64_t m = 0;
    for (int i = 0; i < P.n_prims; ++i)
        if (may_hit(K, rows[i].cx, rows[i].cy, rows[i].cz, rows[i].r2)) m |= 1ull << i;
    return m;
}

// The order in which the render kernel's CULL builds take a launch's blocks: a stable partition of
// 0 .. n_blocks - 1 -- first the blocks with a non-zero mask, ascending, then the blocks with a zero mask, ascending -- and
// in front of it the two counts.  One buffer of BT_ORDER_HEADER + n_blocks words: [0] = n_live, [1] = n_empty, then the order.
// This loop IS the definition; bt_block_order_kernel (bt_kernels.hip) must produce the same words.
#define BT_ORDER_HEADER 2u
BT_HD void block_order(const uint64_t *masks, uint32_t n_blocks, uint32_t *order, uint32_t *header) {
    uint32_t n_live = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) n_live += masks[b] != 0ull ? 1u : 0u;
    uint32_t live = 0, empty = n_live;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        if (masks[b] != 0ull) order[live++] = b;
        else order[empty++] = b;
    }
    header[0] = n_live;
    header[1] = n_blocks - n_live;
}

// What block_mask() reads, besides the rows themselves: the key under which bt_api.cpp keeps a launch's masks, and the block
// order made from them, on the scene handle (compared with memcmp, so it is zeroed before it is filled).  WHOEVER MAKES
// block_geom, block_ref, block_extent, primary_cone OR may_hit READ ANOTHER FIELD OF BtLaunch ADDS IT HERE.  `rows_generation` stands for the rows: bt_api.cpp
// bumps it wherever the table is uploaded.  `stream`: the masks are ordered behind work of that stream only.
struct MaskKey {
    BtV3 cam_cx, cam_cy, cam_cz, cam_t;
    float yfov, xfov, pixel_width, pixel_height;
    float jitter_u_lo, jitter_u_scale, jitter_v_lo, jitter_v_scale;
    int32_t subsample_n, has_focus;
    float focus, aperture;
    BtV3 disk_x, disk_y;
    float one_scale, clip_min;
    uint32_t width, height, tiles_x, tiles_y, tiles_x_magic;
    int32_t slices, sharded;
    uint32_t rank, world;
    int32_t n_prims;
    uint32_t n_blocks;             // the grid: blocks of the launch
    uint32_t valid;                // 0 = no masks held (never equal to a filled key)
    uint64_t rows_generation;
    const void *rows;
    const void *stream;
};
inline void mask_key(MaskKey &k, const BtLaunch &P, uint32_t n_blocks, uint64_t rows_generation, const void *stream) {
    memset(&k, 0, sizeof k);
    k.cam_cx = P.cam_cx; k.cam_cy = P.cam_cy; k.cam_cz = P.cam_cz; k.cam_t = P.cam_t;
    k.yfov = P.yfov; k.xfov = P.xfov; k.pixel_width = P.pixel_width; k.pixel_height = P.pixel_height;
    k.jitter_u_lo = P.jitter_u_lo; k.jitter_u_scale = P.jitter_u_scale;
    k.jitter_v_lo = P.jitter_v_lo; k.jitter_v_scale = P.jitter_v_scale;
    k.subsample_n = P.subsample_n; k.has_focus = P.has_focus;
    k.focus = P.focus; k.aperture = P.aperture;
    k.disk_x = P.disk_x; k.disk_y = P.disk_y;
    k.one_scale = P.one_scale; k.clip_min = P.clip_min;
    k.width = P.width; k.height = P.height; k.tiles_x = P.tiles_x; k.tiles_y = P.tiles_y; k.tiles_x_magic = P.tiles_x_magic;
    k.slices = P.slices; k.sharded = P.sharded;
    k.rank = P.rank; k.world = P.world;
    k.n_prims = P.n_prims;
    k.n_blocks = n_blocks;
    k.valid = 1u;
    k.rows_generation = rows_generation;
    k.rows = (const void *)P.sphere_rows;
    k.stream = stream;
}

} // namespace btcull
