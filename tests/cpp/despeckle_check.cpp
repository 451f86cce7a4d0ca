// despeckle_check.cpp -- stand-alone host program (its own main, never loaded into Python) that runs csrc/bt_despeckle.hpp's host
// loop over the shapes of tests/test_despeckle_host.py; tests/test_despeckle_sanitized.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it.  The frame and the output are heap blocks of exactly their size, so a tap outside
// the frame is a heap-buffer-overflow.  It checks what holds without a reference: every result is finite and non-negative,
// alpha passes through, nothing grows, an unflagged clean pixel comes back bit for bit, a constant frame is never flagged, the
// counts equal what the output shows, and the order statistic equals the one a sort of the gathered neighbours gives.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "../../bendy_tracer_amd/csrc/bt_despeckle.hpp"

namespace {

using btdespeckle::Texel;

uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

bool same(const Texel &a, const Texel &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int check_shape(uint32_t w, uint32_t h, uint32_t radius, uint32_t rank, uint32_t samples, float ratio, bool constant) {
    int bad = 0;
    const size_t n = (size_t)w * h;
    std::unique_ptr<Texel[]> in(new Texel[n]), out(new Texel[n]);
    uint32_t seed = w * 7919u + h * 104729u + radius * 31u + rank;
    for (size_t i = 0; i < n; ++i) {
        float v[4];
        for (float &f : v) f = constant ? 3.25f : std::ldexp(1.0f + (float)(lcg(seed) >> 9) * 0x1p-23f, (int)(lcg(seed) >> 27) - 20);
        in[i] = Texel{v[0], v[1], v[2], 0.5f + v[3] * 0x1p-13f};
    }
    if (!constant) {                                           // the values step 2 is for, at the first and the last pixel and at pixel 256
        const float poison[5] = {NAN, -3.0f, -INFINITY, INFINITY, 3e38f};
        const size_t at[3] = {0, n - 1, 256};
        for (int k = 0; k < 3; ++k)
            if (at[k] < n) in[at[k]] = Texel{poison[k % 5], poison[(k + 1) % 5], poison[(k + 2) % 5], in[at[k]].w};
        if (n > 2) in[1] = Texel{poison[3], poison[4], 1.0f, 1.0f};
    }
    const float max_value = 65536.0f, floor = 0.01f;
    const float fn = (float)samples, cap = max_value * fn, fl = floor * fn;
    uint64_t flagged = 0, sanitised = 0, seen_flagged = 0, seen_sanitised = 0;
    btdespeckle::run_host(in.get(), samples, out.get(), w, h, radius, rank, ratio, floor, max_value, &flagged, &sanitised);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const size_t i = (size_t)y * w + x;
            bool changed;
            const Texel s = btdespeckle::sanitise(in[i], cap, changed);
            const float o[3] = {out[i].x, out[i].y, out[i].z}, c[3] = {s.x, s.y, s.z};
            for (int k = 0; k < 3; ++k)
                if (!std::isfinite(o[k]) || o[k] < 0.0f || o[k] > c[k]) ++bad;
            if (out[i].w != in[i].w) ++bad;
            // the order statistic again, by sorting the neighbours gathered with explicit bounds
            std::vector<float> ys;
            const int R = (int)radius;
            for (int dy = -R; dy <= R; ++dy)
                for (int dx = -R; dx <= R; ++dx) {
                    const int64_t px = (int64_t)x + dx, py = (int64_t)y + dy;
                    if ((dx == 0 && dy == 0) || px < 0 || py < 0 || px >= (int64_t)w || py >= (int64_t)h) continue;
                    ys.push_back(btdespeckle::weigh(in[(size_t)py * w + (size_t)px], cap));
                }
            if (ys.size() != btdespeckle::neighbours(x, y, radius, w, h)) ++bad;
            std::sort(ys.begin(), ys.end(), std::greater<float>());
            bool expect = false;
            Texel want = s;
            if (!ys.empty()) {
                const float lim = btdespeckle::limit(ys[std::min<size_t>(rank, ys.size()) - 1], ratio, fl);
                want = btdespeckle::apply(s, btdespeckle::luminance(s), lim, (uint32_t)ys.size(), expect);
            }
            if (!same(out[i], want)) ++bad;
            if (!expect && !changed && !same(out[i], in[i])) ++bad;
            if (constant && (expect || changed)) ++bad;
            seen_flagged += expect ? 1u : 0u;
            seen_sanitised += changed ? 1u : 0u;
        }
    if (flagged != seen_flagged || sanitised != seen_sanitised) ++bad;
    return bad;
}

} // namespace

int main() {
    const uint32_t shapes[][2] = {{1, 1}, {2, 1}, {1, 2}, {3, 5}, {16, 17}, {45, 35}, {257, 3}, {3, 257}, {24, 32}};
    int bad = 0, runs = 0;
    for (const auto &s : shapes)
        for (uint32_t radius = 1; radius <= 2; ++radius) {
            const uint32_t ranks[] = {1, 2, 3, 4, 5, btdespeckle::max_rank(radius)};      // every selection the header has
            for (uint32_t rank : ranks)
                for (int constant = 0; constant < 2; ++constant) {
                    const uint32_t samples = 1 + (runs % 4);
                    const float ratio = runs % 2 ? 4.0f : 1.0f;
                    const int b = check_shape(s[0], s[1], radius, rank, samples, ratio, constant != 0);
                    if (b) std::printf("%u x %u, radius %u, rank %u, samples %u%s: %d bad\n", s[0], s[1], radius, rank, samples, constant ? ", constant" : "", b);
                    bad += b;
                    ++runs;
                }
        }
    std::printf("%d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
