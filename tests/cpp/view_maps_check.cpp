// view_maps_check.cpp -- stand-alone host program (its own main, never loaded into Python) that runs csrc/bt_view.hpp's maps
// over the pixel sets of tests/test_view_projection.py; tests/test_view_maps_sanitized.py builds it with the host compiler
// under -fsanitize=address,undefined and runs it.  Checks what holds without a reference: every result is finite, and a
// pixel reprojected into its own view comes back to itself.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bendy_tracer_amd/csrc/bt_view.hpp"

namespace {

bt_view make_view(const double L[9], const double T[3], uint32_t w, uint32_t h, uint32_t n) {
    bt_view v{};
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) v.to_world[3 * c + r] = (float)L[3 * r + c];
    for (int k = 0; k < 3; ++k) v.to_world[9 + k] = (float)T[k];
    v.yfov = 0.6f;
    v.xfov = v.yfov * ((float)w / (float)h);
    v.clip_min = 0.01f;
    v.clip_max = 1000.0f;
    v.width = w;
    v.height = h;
    v.subsample_n = n;
    return v;
}

void yaw(const double L[9], double a, double out[9]) {           // L * R_y(a), row-major
    const double c = std::cos(a), s = std::sin(a);
    const double R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) out[3 * r + k] = L[3 * r] * R[k] + L[3 * r + 1] * R[3 + k] + L[3 * r + 2] * R[6 + k];
}

} // namespace

int main() {
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double base[9], turned[9];
    yaw(I, 0.7, base);
    yaw(base, 0.03, turned);
    const double T0[3] = {1.5, -0.75, 4.0}, T1[3] = {1.55, -0.77, 4.03};
    const uint32_t frames[6][2] = {{1, 1}, {16, 17}, {45, 35}, {64, 36}, {768, 512}, {3840, 2160}};
    const float depths[3] = {0.002f, 0.3f, 1.0f};
    long checked = 0;
    int bad = 0;
    for (const auto &f : frames) {
        const uint32_t w = f[0], h = f[1];
        const bool all = (uint64_t)w * h <= 64 * 36;
        std::vector<uint32_t> px;                                // x, y pairs: every pixel, or the border and the two diagonals
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const bool edge = x == 0 || y == 0 || x + 1 == w || y + 1 == h;
                const bool diag = w > 1 && (y == (uint64_t)x * (h - 1) / (w - 1) || y == (uint64_t)(w - 1 - x) * (h - 1) / (w - 1));
                if (all || edge || diag) { px.push_back(x); px.push_back(y); }
            }
        for (uint32_t n : {0u, 2u}) {
            btview::View cur, same, moved;
            const bt_view vc = make_view(base, T0, w, h, n), vm = make_view(turned, T1, w, h, n);
            if (!btview::prepare(vc, cur) || !btview::prepare(vc, same) || !btview::prepare(vm, moved)) {
                std::fprintf(stderr, "prepare refused a valid view\n");
                return 1;
            }
            for (size_t i = 0; i < px.size(); i += 2)
                for (float z : depths) {
                    float a[3], b[3];
                    btview::reproject(cur, same, (float)px[i], (float)px[i + 1], z, a);
                    btview::reproject(cur, moved, (float)px[i], (float)px[i + 1], z, b);
                    ++checked;
                    const bool ok = std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]) && std::isfinite(b[0]) &&
                                    std::isfinite(b[1]) && std::isfinite(b[2]) && std::fabs(a[0] - (float)px[i]) <= 5e-3f &&
                                    std::fabs(a[1] - (float)px[i + 1]) <= 5e-3f;
                    if (!ok && bad++ < 5)
                        std::fprintf(stderr, "%ux%u n=%u pixel (%u, %u) z=%g: (%g, %g, %g) / (%g, %g, %g)\n", w, h, n, px[i], px[i + 1], z,
                                     a[0], a[1], a[2], b[0], b[1], b[2]);
                }
        }
    }
    bt_view singular = make_view(I, T0, 4, 4, 0);
    singular.to_world[8] = 0.0f;
    btview::View s;
    if (btview::prepare(singular, s)) { std::fprintf(stderr, "prepare accepted a singular view\n"); return 1; }
    std::printf("view_maps_check: %ld reprojections, %d bad\n", checked, bad);
    return bad ? 1 : 0;
}
