// glare_check.cpp -- stand-alone host program (its own main, never loaded into Python) that runs csrc/bt_glare.hpp's host loop
// over the shapes of tests/test_glare_host.py; tests/test_glare_sanitized.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it.  The frame, the output and every plane of the pyramid are heap blocks of exactly
// their size, so a tap outside a plane is a heap-buffer-overflow.  It checks what holds without a reference: every result is
// finite and non-negative, alpha passes through, strength 0 returns the sanitised mean, a constant frame keeps every plane
// constant, and the planes equal those of a two-pass (x, then y) form built from the header's one-axis functions.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../bendy_tracer_amd/csrc/bt_glare.hpp"

namespace {

using btglare::Texel;

uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

float channel(const Texel &t, int c) { return c == 0 ? t.x : c == 1 ? t.y : c == 2 ? t.z : t.w; }
bool same(const Texel &a, const Texel &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// one axis at a time, each pass into a block of its own
std::vector<Texel> down_two_pass(const std::vector<Texel> &src, uint32_t sw, uint32_t sh) {
    const uint32_t dw = btglare::half_side(sw), dh = btglare::half_side(sh);
    std::vector<Texel> mid((size_t)dw * sh), dst((size_t)dw * dh);
    for (uint32_t y = 0; y < sh; ++y)
        for (uint32_t i = 0; i < dw; ++i) {
            const Texel *row = &src[(size_t)y * sw];
            mid[(size_t)y * dw + i] = btglare::down4(row[btglare::down_tap(i, 0, sw)], row[btglare::down_tap(i, 1, sw)],
                                                     row[btglare::down_tap(i, 2, sw)], row[btglare::down_tap(i, 3, sw)]);
        }
    for (uint32_t j = 0; j < dh; ++j)
        for (uint32_t i = 0; i < dw; ++i)
            dst[(size_t)j * dw + i] =
                btglare::down4(mid[(size_t)btglare::down_tap(j, 0, sh) * dw + i], mid[(size_t)btglare::down_tap(j, 1, sh) * dw + i],
                               mid[(size_t)btglare::down_tap(j, 2, sh) * dw + i], mid[(size_t)btglare::down_tap(j, 3, sh) * dw + i]);
    return dst;
}

std::vector<Texel> up_two_pass(const std::vector<Texel> &c, uint32_t cw, uint32_t ch, uint32_t w, uint32_t h) {
    std::vector<Texel> mid((size_t)w * ch), dst((size_t)w * h);
    for (uint32_t y = 0; y < ch; ++y)
        for (uint32_t x = 0; x < w; ++x) mid[(size_t)y * w + x] = btglare::up2(c[(size_t)y * cw + btglare::up_far(x, cw)], c[(size_t)y * cw + (x >> 1)]);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) dst[(size_t)y * w + x] = btglare::up2(mid[(size_t)btglare::up_far(y, ch) * w + x], mid[(size_t)(y >> 1) * w + x]);
    return dst;
}

int check_shape(uint32_t w, uint32_t h, uint32_t levels, uint32_t samples, float spread, float strength, bool constant) {
    int bad = 0;
    const size_t n = (size_t)w * h;
    std::unique_ptr<Texel[]> in(new Texel[n]), out(new Texel[n]), out0(new Texel[n]);
    uint32_t seed = w * 7919u + h * 104729u + levels;
    for (size_t i = 0; i < n; ++i) {
        float v[4];
        for (float &f : v) f = constant ? 3.25f : std::ldexp(1.0f + (float)(lcg(seed) >> 9) * 0x1p-23f, (int)(lcg(seed) >> 27) - 20);
        in[i] = Texel{v[0], v[1], v[2], 0.5f + v[3] * 0x1p-13f};
    }
    if (!constant) {                                           // the values step 1 is for, at the first and the last pixel and at pixel 256
        const float poison[5] = {NAN, -3.0f, -INFINITY, INFINITY, 3e38f};
        const size_t at[3] = {0, n - 1, 256};
        for (int k = 0; k < 3; ++k)
            if (at[k] < n) in[at[k]] = Texel{poison[k % 5], poison[(k + 1) % 5], poison[(k + 2) % 5], in[at[k]].w};
        if (n > 2) in[1] = Texel{poison[3], poison[4], 1.0f, 1.0f};
    }
    const float max_value = 65536.0f, r = 1.0f / (float)samples;
    std::vector<std::vector<Texel>> planes;
    btglare::run_host(in.get(), samples, out.get(), w, h, levels, spread, strength, max_value, &planes);
    btglare::run_host(in.get(), samples, out0.get(), w, h, levels, spread, 0.0f, max_value);
    const uint32_t L = btglare::effective_levels(levels, w, h);
    if (planes.size() != L) ++bad;
    for (size_t i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(channel(out[i], c)) || channel(out[i], c) < 0.0f) ++bad;
        if (out[i].w != in[i].w || out0[i].w != in[i].w) ++bad;
        Texel s = btglare::sanitise(in[i], r, max_value);
        s.w = in[i].w;
        if (!same(out0[i], s)) ++bad;
        if (constant && L > 0 && std::fabs(out[i].x - 3.25f * r) > 3.25f * r * (float)(2 * L + 1) * 0x1p-23f) ++bad;
    }
    if (L == 0) return bad;
    // the same planes, one axis at a time
    float wk[BT_GLARE_MAX_LEVELS + 1];
    btglare::level_weights(L, spread, wk);
    std::vector<std::vector<Texel>> D(L + 1);
    std::vector<uint32_t> pw(L + 1), ph(L + 1);
    pw[0] = w;
    ph[0] = h;
    D[0].resize(n);
    for (size_t i = 0; i < n; ++i) D[0][i] = btglare::sanitise(in[i], r, max_value);
    for (uint32_t k = 1; k <= L; ++k) {
        D[k] = down_two_pass(D[k - 1], pw[k - 1], ph[k - 1]);
        pw[k] = btglare::half_side(pw[k - 1]);
        ph[k] = btglare::half_side(ph[k - 1]);
    }
    std::vector<Texel> A = D[L];
    for (Texel &t : A) t = btglare::scale(t, wk[L]);
    for (uint32_t k = L;; --k) {
        if (planes[k - 1].size() != A.size()) return bad + 1;
        for (size_t i = 0; i < A.size(); ++i) {
            if (!same(planes[k - 1][i], A[i])) ++bad;
            if (constant && !same(A[i], A[0])) ++bad;
        }
        if (k == 1) break;
        const std::vector<Texel> u = up_two_pass(A, pw[k], ph[k], pw[k - 1], ph[k - 1]);
        A = D[k - 1];
        for (size_t i = 0; i < A.size(); ++i) A[i] = btglare::accumulate(A[i], wk[k - 1], u[i]);
    }
    const std::vector<Texel> G = up_two_pass(A, pw[1], ph[1], w, h);
    for (size_t i = 0; i < n; ++i)
        if (!same(out[i], btglare::composite(D[0][i], G[i], strength, in[i].w))) ++bad;
    return bad;
}

} // namespace

int main() {
    const uint32_t shapes[][2] = {{1, 1}, {2, 1}, {1, 2}, {3, 5}, {16, 17}, {45, 35}, {257, 3}, {3, 257}, {300, 200}};
    const uint32_t levels[] = {0, 1, 2, 3, 6, 16};
    int bad = 0, runs = 0;
    for (const auto &s : shapes)
        for (uint32_t lv : levels)
            for (int constant = 0; constant < 2; ++constant) {
                const uint32_t samples = 1 + (runs % 4);
                const int b = check_shape(s[0], s[1], lv, samples, runs % 3 == 0 ? 0.5f : runs % 3 == 1 ? 1.0f : 2.0f, constant ? 1.0f : 0.3f, constant != 0);
                if (b) std::printf("%u x %u, levels %u, samples %u%s: %d bad\n", s[0], s[1], lv, samples, constant ? ", constant" : "", b);
                bad += b;
                ++runs;
            }
    std::printf("%d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
