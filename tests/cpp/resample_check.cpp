// resample_check.cpp -- stand-alone host program (its own main, never loaded into Python) that runs csrc/bt_resample.hpp's host
// loop over the shapes of tests/test_resample_host.py; tests/test_resample_sanitized.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it.  The frame, the intermediate plane and the output are heap blocks of exactly their
// size, so a tap outside a plane is a heap-buffer-overflow.  It checks what holds without a reference: every result is finite
// and with the clamp non-negative, alpha is the nearest input pixel's, tent and lanczos3 at equal sizes return the sanitised
// mean, a constant frame comes back within T_x + T_y ulps and the rounding of the weights, every tile's staged span holds
// each of its clamped taps, and the output equals a per-texel form that filters a column of horizontally filtered rows.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../bendy_tracer_amd/csrc/bt_resample.hpp"

namespace {

using btresample::Axis;
using btresample::Texel;

uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

float channel(const Texel &t, int c) { return c == 0 ? t.x : c == 1 ? t.y : c == 2 ? t.z : t.w; }
bool same(const Texel &a, const Texel &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// a table as the kernels see it: first taps that never decrease, rows of `taps`, and every tile's clamped taps inside its span
int check_axis(const Axis &ax, uint32_t tile) {
    int bad = 0;
    if (ax.first.size() != ax.dst || ax.nearest.size() != ax.dst || ax.weights.size() != (size_t)ax.dst * ax.taps || ax.taps == 0 ||
        ax.taps > BT_RESAMPLE_MAX_TAPS)
        return 1;
    for (uint32_t i = 0; i < ax.dst; ++i) {
        if (i && ax.first[i] < ax.first[i - 1]) ++bad;
        if (ax.nearest[i] >= ax.src) ++bad;
        double sum = 0.0;
        for (uint32_t t = 0; t < ax.taps; ++t) sum += (double)ax.weights[(size_t)i * ax.taps + t];
        if (std::fabs(sum - 1.0) > (double)ax.taps * 0x1p-23) ++bad;
        uint32_t origin;
        const uint32_t span = ax.reach_of(i - i % tile, tile, origin);
        for (uint32_t t = 0; t < ax.taps; ++t) {
            const uint32_t p = btresample::clamp_index((int64_t)ax.first[i] + t, ax.src);
            if (p < origin || p - origin >= span) ++bad;
        }
    }
    if (ax.widest(tile) > ax.src) ++bad;
    return bad;
}

int check_shape(uint32_t w, uint32_t h, uint32_t W, uint32_t H, int filter, uint32_t samples, int clamp_negative, bool constant) {
    int bad = 0;
    const size_t n = (size_t)w * h, N = (size_t)W * H;
    std::unique_ptr<Texel[]> in(new Texel[n]), out(new Texel[N]), plane(new Texel[(size_t)W * h]);
    uint32_t seed = w * 7919u + h * 104729u + W * 31u + H + (uint32_t)filter;
    for (size_t i = 0; i < n; ++i) {
        float v[4];
        for (float &f : v) f = constant ? 3.25f : std::ldexp(1.0f + (float)(lcg(seed) >> 9) * 0x1p-23f, (int)(lcg(seed) >> 27) - 20);
        in[i] = Texel{v[0], v[1], v[2], constant ? 1.0f : 0.5f + v[3] * 0x1p-13f};
    }
    if (!constant) {                                           // the values step 1 is for, at the first and the last pixel and at pixel 256
        const float poison[5] = {NAN, -3.0f, -INFINITY, INFINITY, 3e38f};
        const size_t at[3] = {0, n - 1, 256};
        for (int k = 0; k < 3; ++k)
            if (at[k] < n) in[at[k]] = Texel{poison[k % 5], poison[(k + 1) % 5], poison[(k + 2) % 5], in[at[k]].w};
        if (n > 2) in[1] = Texel{poison[3], poison[4], 1.0f, 1.0f};
    }
    const float max_value = 65536.0f, r = 1.0f / (float)samples;
    Axis ax, ay;
    btresample::build_axis(ax, w, W, filter);
    btresample::build_axis(ay, h, H, filter);
    bad += check_axis(ax, 32) + check_axis(ay, 32);
    if (bad) return bad;
    btresample::run_host(in.get(), samples, w, h, out.get(), W, H, ax, ay, max_value, clamp_negative, plane.get());
    double e = 0.0;                                            // how far the rows' float32 weights are from summing to 1
    for (const Axis *a : {&ax, &ay}) {
        double worst = 0.0;
        for (uint32_t i = 0; i < a->dst; ++i) {
            double sum = 0.0;
            for (uint32_t t = 0; t < a->taps; ++t) sum += (double)a->weights[(size_t)i * a->taps + t];
            worst = std::fmax(worst, std::fabs(sum - 1.0));
        }
        e += worst;
    }
    const float c = 3.25f * r;
    const double ulp = (double)std::nextafter(c, INFINITY) - (double)c;
    for (uint32_t j = 0; j < H; ++j)
        for (uint32_t i = 0; i < W; ++i) {
            const Texel &o = out[(size_t)j * W + i];
            for (int ch = 0; ch < 3; ++ch) {
                if (!std::isfinite(channel(o, ch)) || (clamp_negative && channel(o, ch) < 0.0f)) ++bad;
                if (constant && std::fabs((double)channel(o, ch) - (double)c) > (double)(ax.taps + ay.taps) * ulp + 1.01 * e * (double)c) ++bad;
            }
            if (o.w != in[(size_t)ay.nearest[j] * w + ax.nearest[i]].w) ++bad;
            if (w == W && h == H && (filter == 1 || filter == 3)) {
                Texel s = btglare::sanitise(in[(size_t)j * w + i], r, max_value);
                s.w = in[(size_t)j * w + i].w;
                if (!same(o, s)) ++bad;
            }
            // the same texel, one output at a time: the rows it takes are filtered along x, then the column of results along y
            std::vector<Texel> column(ay.taps);
            for (uint32_t t = 0; t < ay.taps; ++t) {
                const Texel *row = in.get() + (size_t)btresample::clamp_index((int64_t)ay.first[j] + t, h) * w;
                column[t] = btresample::filter_texel<Texel>([&](uint32_t p) { return btglare::sanitise(row[p], r, max_value); },
                                                            &ax.weights[(size_t)i * ax.taps], ax.first[i], ax.taps, w);
            }
            const int64_t base = ay.first[j];
            const Texel acc = btresample::filter_texel<Texel>(
                [&](uint32_t p) {
                    // position p of the y axis is tap clamp^-1: find the first tap that clamps to p
                    for (uint32_t t = 0; t < ay.taps; ++t)
                        if (btresample::clamp_index(base + t, h) == p) return column[t];
                    return Texel{NAN, NAN, NAN, NAN};
                },
                &ay.weights[(size_t)j * ay.taps], ay.first[j], ay.taps, h);
            if (!same(o, btresample::finish(acc, clamp_negative, o.w))) ++bad;
        }
    return bad;
}

} // namespace

int main() {
    const uint32_t shapes[][4] = {{1, 1, 1, 1},     {1, 1, 5, 3},     {5, 3, 1, 1},   {3, 5, 7, 2},     {16, 17, 45, 35}, {45, 35, 16, 17},
                                  {45, 35, 45, 35}, {257, 3, 64, 3},  {3, 257, 3, 64}, {64, 36, 128, 72}, {300, 200, 77, 51}, {2100, 2, 100, 1}};
    int bad = 0, runs = 0;
    for (const auto &s : shapes)
        for (int filter = 0; filter < BT_RESAMPLE_FILTERS; ++filter)
            for (int constant = 0; constant < 2; ++constant) {
                const uint32_t samples = 1 + 2 * (runs % 2);
                const int clamp_negative = constant ? 0 : (runs / 2) % 2;
                const int b = check_shape(s[0], s[1], s[2], s[3], filter, samples, clamp_negative, constant != 0);
                if (b)
                    std::printf("%u x %u -> %u x %u, %s, samples %u%s: %d bad\n", s[0], s[1], s[2], s[3], btresample::filter_name(filter), samples,
                                constant ? ", constant" : "", b);
                bad += b;
                ++runs;
            }
    std::printf("%d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
