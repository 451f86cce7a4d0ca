// compare_check.cpp -- a stand-alone program (its own main, nothing of it loaded into Python) that runs csrc/bt_compare.hpp's
// host loop under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_compare_sanitized.py builds it): the whole stage
// over frames whose planes are heap blocks of exactly their size, non-finite and 3e38 pixels included, and the tail at three
// fractions; then, over those shapes and a sweep of further sides, that every clamped tap of every tile lies inside the 26 x 26
// stage at the entry the kernel reads.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../../bendy_tracer_amd/csrc/bt_compare.hpp"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
double uniform() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

int run(uint32_t w, uint32_t h, int variant) {
    const size_t n = (size_t)w * h;
    std::unique_ptr<btcompare::Texel[]> X(new btcompare::Texel[n]), Y(new btcompare::Texel[n]);
    std::unique_ptr<float[]> E(new float[n]);
    std::unique_ptr<btcompare::Pair[]> V(new btcompare::Pair[n]);
    std::unique_ptr<double[]> S(new double[n]);
    for (size_t p = 0; p < n; ++p) {
        const float y0 = (float)std::exp2(40.0 * uniform() - 20.0), y1 = (float)std::exp2(40.0 * uniform() - 20.0), y2 = (float)uniform();
        Y[p] = btcompare::Texel{y0, y1, y2, 1.0f};
        X[p] = btcompare::Texel{y0 * (float)(0.2 + 1.6 * uniform()), y1, y2 * (float)(2.0 * uniform() - 0.5), 0.5f};
    }
    const size_t spots[3] = {0, n - 1, n > 256 ? 256 : n / 2};
    for (int s = 0; s < 3; ++s) {
        if (variant == 1) (s % 2 ? Y : X)[spots[s]].y = s == 0 ? NAN : s == 1 ? INFINITY : -INFINITY;
        if (variant == 2) (s % 2 ? Y : X)[spots[s]].x = 3e38f;
    }
    btcompare::Sums sums;
    btcompare::run_host(X.get(), variant == 2 ? 1 : 3, Y.get(), variant == 2 ? 1 : 4, w, h, variant ? 1e-4 : 0.01, E.get(), V.get(), S.get(), sums);
    int bad = 0;
    if (sums.valid + sums.nonfinite != n || sums.pixels != n) ++bad;
    if (variant == 1 && sums.nonfinite == 0) ++bad;
    if (!(sums.se >= 0.0) || !(sums.re >= 0.0) || !std::isfinite(sums.s) || sums.max_index >= n) ++bad;
    for (size_t p = 0; p < n; ++p)
        if (!std::isfinite(E[p]) || !std::isfinite(S[p]) || !(V[p].x >= 0.0 && V[p].x <= 1.0) || !(V[p].y >= 0.0 && V[p].y <= 1.0)) ++bad;
    const double fractions[3] = {0.01, 0.5, 1.0};
    double last = 0.0;
    for (double f : fractions) {
        double share = -1.0;
        float T = -1.0f;
        btcompare::tail_host(E.get(), w, h, sums.valid, f, share, T);
        if (!(share >= last - 1e-12) || !(share <= 1.0 + 1e-12) || !(T >= 0.0f)) ++bad;
        last = share;
        (void)btcompare::map_pixel(T, 1.0f);
    }
    return bad;
}

// every tap of every pixel of every tile of an axis of n texels, against the stage entry the kernel reads for it
long stage_axis(uint32_t n, long &taps) {
    long bad = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += BT_COMPARE_TILE)
        for (uint32_t l = 0; l < BT_COMPARE_TILE; ++l)          // threads outside the frame read the stage too
            for (uint32_t k = 0; k < BT_COMPARE_TAPS; ++k) {
                const uint32_t entry = l + k;
                ++taps;
                if (entry >= BT_COMPARE_SPAN) ++bad;
                const uint32_t texel = btcompare::stage_texel(i0, entry, n);
                if (texel >= n) ++bad;
                if (i0 + l < n && texel != btcompare::clamp_index((int64_t)(i0 + l) + k - 5, n)) ++bad;
            }
    return bad;
}

} // namespace

int main() {
    const uint32_t shapes[][2] = {{1, 1}, {5, 1}, {1, 5}, {11, 11}, {16, 16}, {17, 16}, {16, 17}, {33, 33}, {45, 35}, {64, 36}};
    long bad = 0, frames = 0, taps = 0;
    for (const auto &s : shapes)
        for (int variant = 0; variant < 3; ++variant) {
            bad += run(s[0], s[1], variant);
            ++frames;
        }
    for (const auto &s : shapes) bad += stage_axis(s[0], taps) + stage_axis(s[1], taps);
    for (uint32_t n = 1; n <= 300; ++n) bad += stage_axis(n, taps);
    const uint32_t far[] = {1048595u, 0x7fffffffu - 20u, 0x7fffffffu};
    for (uint32_t n : far) {                                     // the last tiles of the longest sides
        const uint32_t first = (n - 1) / BT_COMPARE_TILE * BT_COMPARE_TILE;
        for (uint32_t i0 : {0u, first - BT_COMPARE_TILE, first})
            for (uint32_t a = 0; a < BT_COMPARE_SPAN; ++a) {
                ++taps;
                if (btcompare::stage_texel(i0, a, n) >= n) ++bad;
            }
    }
    std::printf("%ld frames, %ld taps, %ld bad\n", frames, taps, bad);
    return bad ? 1 : 0;
}
