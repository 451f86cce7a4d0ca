// upscale_check.cpp -- stand-alone host program (its own main, never loaded into Python) that runs csrc/bt_upscale.hpp's host loop
// over the shapes of tests/test_upscale_host.py and two one-texel-wide frames; tests/test_upscale_sanitized.py builds it with the
// host compiler under -fsanitize=address,undefined and runs it.  The frames, the prepared planes and the output are heap blocks
// of exactly their size, so a tap outside a plane is a heap-buffer-overflow.  It checks what holds without a reference: every
// result is finite, non-negative and no larger than the largest prepared colour, alpha is the nearest texel's, the counts equal
// the tiers seen, a frame without guides never leaves tier 1 -- and, for the staged kernel, that every clamped tap of every
// 16 x 16 tile of outputs lies inside the 19 x 19 span of source texels the tile stages, at the position the kernel reads.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../bendy_tracer_amd/csrc/bt_upscale.hpp"

namespace {

using btupscale::Texel;

uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
float unit(uint32_t &s) { return (float)(lcg(s) >> 8) * 0x1p-24f; }

const float kPoison[5] = {NAN, -3.0f, -INFINITY, INFINITY, 3e38f};

// a frame of sums of `n` samples: kind 0 colour (log-normal), 1 albedo, 2 normal (one in eight a miss), 3 depth; a few regions
// so that taps match here and miss there
void fill(Texel *f, uint32_t w, uint32_t h, int kind, uint32_t n, uint32_t seed, bool poison) {
    const size_t texels = (size_t)w * h;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const uint32_t region = ((x * 4u) / w + 2u * ((y * 4u) / h)) % 5u;
            uint32_t s = kind == 0 ? seed + (uint32_t)(y * w + x) * 2654435761u : seed + region * 97u;
            float v[3];
            if (kind == 0)
                for (float &c : v) c = std::ldexp(1.0f + unit(s), (int)(lcg(s) >> 27) - 16);
            else if (kind == 1)
                for (float &c : v) c = unit(s);
            else if (kind == 2) {
                for (float &c : v) c = unit(s) * 2.0f - 1.0f;
                if (region == 0) v[0] = v[1] = v[2] = 0.0f;
            } else
                v[0] = v[1] = v[2] = 0.5f + 19.5f * unit(s);
            f[(size_t)y * w + x] = Texel{v[0] * (float)n, v[1] * (float)n, v[2] * (float)n, 0.5f + unit(s)};
        }
    if (poison) {
        const size_t at[3] = {0, texels - 1, 256};
        for (int k = 0; k < 3; ++k)
            if (at[k] < texels) f[at[k]] = Texel{kPoison[(k + kind) % 5], kPoison[(k + kind + 1) % 5], kPoison[(k + kind + 2) % 5], f[at[k]].w};
    }
}

// the staged kernel's footprint: tile (i0, j0) stages the texels clamp(first[i0] + a), a = 0 .. 18, of each axis, and output i
// reads entry first[i] - first[i0] + t of it for tap t
int check_span(const btupscale::Axis &ax) {
    int bad = 0;
    for (uint64_t i0 = 0; i0 < ax.dst; i0 += BT_UPSCALE_TILE)
        for (uint32_t i = (uint32_t)i0; i < ax.dst && i < i0 + BT_UPSCALE_TILE; ++i)
            for (int t = 0; t < 4; ++t) {
                const int64_t entry = (int64_t)ax.first[i] - ax.first[i0] + t;
                if (entry < 0 || entry >= BT_UPSCALE_SPAN) {
                    ++bad;
                    continue;
                }
                if (btupscale::clamp_index((int64_t)ax.first[i0] + entry, ax.src) != btupscale::clamp_index((int64_t)ax.first[i] + t, ax.src)) ++bad;
            }
    return bad;
}

int check_shape(uint32_t w, uint32_t h, uint32_t W, uint32_t H, int mask, uint32_t samples, uint32_t guide_samples, bool other) {
    int bad = 0;
    const size_t lo_n = (size_t)w * h, hi_n = (size_t)W * H;
    std::unique_ptr<Texel[]> colour(new Texel[lo_n]), out(new Texel[hi_n]), planes(new Texel[3 * lo_n]);
    std::unique_ptr<Texel[]> lo[3], hi[3];
    const uint32_t seed = w * 7919u + h * 104729u + W * 31u + H;
    fill(colour.get(), w, h, 0, samples, seed, true);
    for (int k = 0; k < 3; ++k)
        if (mask >> k & 1) {
            lo[k].reset(new Texel[lo_n]);
            hi[k].reset(new Texel[hi_n]);
            fill(lo[k].get(), w, h, k + 1, guide_samples, seed + 11u, true);
            fill(hi[k].get(), W, H, k + 1, guide_samples, seed + 11u, true);
        }
    const float r = 1.0f / (float)guide_samples;
    const btupscale::Guides gl{lo[0].get(), lo[1].get(), lo[2].get(), r, r, r}, gh{hi[0].get(), hi[1].get(), hi[2].get(), r, r, r};
    btupscale::Weights P;
    P.sigma_depth = other ? 0.3f : 0.1f;
    P.k_a = 1.0f / ((other ? 0.03f : 0.1f) * (other ? 0.03f : 0.1f));
    P.min_weight = other ? 0.1f : 0.01f;
    P.squarings = other ? 0u : 3u;
    const float max_value = other ? 100.0f : 65536.0f;
    btupscale::Axis ax, ay;
    btupscale::build_axis(ax, w, W);
    btupscale::build_axis(ay, h, H);
    bad += check_span(ax) + check_span(ay);
    uint64_t tier2 = ~0ull, tier3 = ~0ull;
    btupscale::run_host(colour.get(), samples, w, h, gl, gh, out.get(), W, H, ax, ay, P, max_value, planes.get(), &tier2, &tier3);
    float largest = 0.0f;
    for (size_t i = 0; i < lo_n; ++i) {
        const float c[3] = {planes[i].x, planes[i].y, planes[i].z};
        for (float v : c) {
            if (!(v >= 0.0f && v <= max_value)) ++bad;
            if (v > largest) largest = v;
        }
    }
    for (uint32_t j = 0; j < H; ++j)
        for (uint32_t i = 0; i < W; ++i) {
            const Texel o = out[(size_t)j * W + i];
            const float c[3] = {o.x, o.y, o.z};
            // a weighted mean of non-negative values, each quotient rounded once
            for (float v : c)
                if (!std::isfinite(v) || v < 0.0f || v > largest * 1.0001f) ++bad;
            const Texel near = colour[(size_t)ay.nearest[j] * w + ax.nearest[i]];
            if (std::memcmp(&o.w, &near.w, sizeof(float)) != 0) ++bad;
        }
    if (tier2 + tier3 > hi_n) ++bad;
    if (mask == 0 && (tier2 || tier3)) ++bad;                  // without guides D1 is the bilinear weights' sum, 1
    return bad;
}

} // namespace

int main() {
    const uint32_t shapes[][4] = {{1, 1, 1, 1},     {1, 1, 5, 3},     {3, 5, 7, 9},     {8, 8, 16, 16},   {8, 8, 32, 32},  {2, 2, 64, 64},
                                  {16, 17, 45, 35}, {17, 16, 33, 33}, {45, 35, 45, 35}, {64, 36, 128, 72}, {1, 3, 1, 257}, {3, 1, 257, 1}};
    int bad = 0, runs = 0;
    for (const auto &s : shapes)
        for (int mask = 0; mask < 8; ++mask) {
            const uint32_t samples = runs % 2 ? 3u : 1u, guide_samples = runs % 3 ? 4u : 1u;
            const int b = check_shape(s[0], s[1], s[2], s[3], mask, samples, guide_samples, runs % 4 >= 2);
            if (b) std::printf("%u x %u -> %u x %u, guides %d, samples %u / %u: %d bad\n", s[0], s[1], s[2], s[3], mask, samples, guide_samples, b);
            bad += b;
            ++runs;
        }
    // the footprint over many ratios, sides that are no multiple of the tile included
    for (uint32_t src = 1; src <= 70; ++src)
        for (uint32_t dst = src; dst <= 4 * src + 40; dst += 1 + dst / 9) {
            btupscale::Axis a;
            btupscale::build_axis(a, src, dst);
            const int b = check_span(a);
            if (b) std::printf("axis %u -> %u: %d taps outside the staged span\n", src, dst, b);
            bad += b;
            ++runs;
        }
    std::printf("%d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
