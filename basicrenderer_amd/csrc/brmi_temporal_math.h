// brmi_temporal_math.h -- the temporal resolve's arithmetic: the bounded colour space, the neighbourhood box, the dilated velocity, the reprojection, the
// history sample, the clamp and the blend.  Plain C++ for host and device: brmi_temporal.hip's kernel and tests/temporal_main.cpp compile it.
//
// The reference's resolvers are vendor binaries; this stage is the project's own.  Arithmetic as in brmi_display_math.h: IEEE fp32 without contraction, a * b + c is
// two roundings, division is the correctly rounded one, min / max through fminf / fmaxf (which return the other operand for a NaN), and every value that is STORED
// (the w-space neighbourhood, the output) is rounded to half where it is stored.  No transcendental function: kernel, host program and the numpy restatement
// (tests/temporal_ref.py) compute the same bits.
#ifndef BRMI_TEMPORAL_MATH_H
#define BRMI_TEMPORAL_MATH_H

#include "brmi_display_math.h"

namespace brmi {
namespace temporal {

using display::rgb;
using display::half_bits;
using display::half_value;

constexpr uint32_t kDepthEmptyBits = 0x7F7FFFFFu;      // the linear-depth surface's "empty" word (FLT_MAX): farther than any depth the rasteriser writes
constexpr float kMinInverse = 1.52587890625e-05f;      // 2^-16: the smallest 1 - max(r) the inverse divides by (w of 4095 and more rounds to the half 1.0)
constexpr float kMaxHalf = 65504.0f;

BRMI_HD float max3(rgb c) { return fmaxf(fmaxf(c.r, c.g), c.b); }
BRMI_HD bool finite3(rgb c) { return isfinite(c.r) && isfinite(c.g) && isfinite(c.b); }
BRMI_HD rgb unpack_rgb(uint32_t lo, uint32_t hi) { return rgb{half_value(lo & 0xFFFFu), half_value(lo >> 16), half_value(hi & 0xFFFFu)}; }

// w(c) = c / (1 + max(c.r, c.g, c.b)): maps [0, inf) into [0, 1), so that one firefly cannot own a box or a blend
BRMI_HD rgb to_w(rgb c) {
    const float d = 1.0f + max3(c);
    return rgb{c.r / d, c.g / d, c.b / d};
}
// the neighbourhood holds w(c) as halves: (r | g << 16, b)
BRMI_HD void to_w_halves(uint32_t lo, uint32_t hi, uint32_t& wlo, uint32_t& whi) {
    const rgb w = to_w(unpack_rgb(lo, hi));
    wlo = half_bits(w.r) | (half_bits(w.g) << 16); whi = half_bits(w.b);
}
// the inverse: c = r / (1 - max(r)), the divisor kept at 2^-16 and the result at the largest half (a w-space half can be exactly 1)
BRMI_HD float from_w_channel(float r, float m) { return fminf(r / fmaxf(1.0f - m, kMinInverse), kMaxHalf); }

struct Box { rgb lo, hi; };
BRMI_HD void box_start(Box& b, rgb w) { b.lo = w; b.hi = w; }
BRMI_HD void box_add(Box& b, rgb w) {
    b.lo = rgb{fminf(b.lo.r, w.r), fminf(b.lo.g, w.g), fminf(b.lo.b, w.b)};
    b.hi = rgb{fmaxf(b.hi.r, w.r), fmaxf(b.hi.g, w.g), fmaxf(b.hi.b, w.b)};
}
BRMI_HD float clamp_channel(float h, float lo, float hi) { return fminf(fmaxf(h, lo), hi); }

// the closest of the nine: strictly smaller wins, so the first in row-major order keeps a tie (and a NaN depth never wins)
BRMI_HD bool closer(float depth, float best) { return depth < best; }

// Reprojection.  mv = ndc_now - ndc_prev of the unjittered matrices; NDC y points up, rows point down.  (x, y) is the previous position of the pixel's centre in
// texel coordinates (centre of texel 0 at 0): the history is present only where 0 <= x <= W - 1 and 0 <= y <= H - 1, i.e. where every tap with a weight is
// inside the frame.  A NaN or infinite motion vector fails the comparisons.
struct Tap { uint32_t x0, x1, y0, y1; float fx, fy; bool inside; };
BRMI_HD Tap tap_of(uint32_t px, uint32_t py, float mvx, float mvy, uint32_t W, uint32_t H) {
    Tap t{};
    const float prevX = ((float)px + 0.5f) - (0.5f * mvx) * (float)W, prevY = ((float)py + 0.5f) + (0.5f * mvy) * (float)H;
    const float x = prevX - 0.5f, y = prevY - 0.5f;
    t.inside = x >= 0.0f && x <= (float)(W - 1u) && y >= 0.0f && y <= (float)(H - 1u);
    if (!t.inside) return t;
    const float x0f = floorf(x), y0f = floorf(y);      // the footprint and weights of display::bilinear_of, in texel coordinates
    t.fx = x - x0f; t.fy = y - y0f;
    t.x0 = (uint32_t)x0f; t.y0 = (uint32_t)y0f;
    t.x1 = t.x0 + 1u < W ? t.x0 + 1u : W - 1u; t.y1 = t.y0 + 1u < H ? t.y0 + 1u : H - 1u;      // (clamped only where the weight is zero)
    return t;
}
BRMI_HD rgb tap_mix(rgb t00, rgb t10, rgb t01, rgb t11, float fx, float fy) {
    return rgb{display::bilinear_mix(t00.r, t10.r, t01.r, t11.r, fx, fy), display::bilinear_mix(t00.g, t10.g, t01.g, t11.g, fx, fy), display::bilinear_mix(t00.b, t10.b, t01.b, t11.b, fx, fy)};
}

// The output's two words with a history sample `h` (linear, finite): clamp w(h) into the box, blend towards w(current), invert, round to half.  `cw` is the centre of
// the neighbourhood (halves already), `alphaBits` the current pixel's.
BRMI_HD void resolve_words(rgb h, rgb cw, const Box& box, float blend, uint32_t alphaBits, uint32_t& lo, uint32_t& hi) {
    const rgb hw = to_w(h);
    const rgb hc{clamp_channel(hw.r, box.lo.r, box.hi.r), clamp_channel(hw.g, box.lo.g, box.hi.g), clamp_channel(hw.b, box.lo.b, box.hi.b)};
    const rgb r{hc.r + blend * (cw.r - hc.r), hc.g + blend * (cw.g - hc.g), hc.b + blend * (cw.b - hc.b)};
    const float m = max3(r);
    lo = half_bits(from_w_channel(r.r, m)) | (half_bits(from_w_channel(r.g, m)) << 16);
    hi = half_bits(from_w_channel(r.b, m)) | (alphaBits << 16);
}

// One pixel from whole images, the way the kernel computes it; `load_*` take clamped pixel coordinates.  The host program's loop and the kernel's documentation.
template <typename Hdr, typename Depth, typename Motion, typename History>
BRMI_HD void resolve_pixel(uint32_t px, uint32_t py, uint32_t W, uint32_t H, float blend, bool haveHistory, Hdr load_hdr, Depth load_depth, Motion load_motion, History load_history,
                           uint32_t& lo, uint32_t& hi) {
    Box box{}; rgb cw{}; float best = 0.0f; uint32_t bx = 0u, by = 0u;
    for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
        const int sx = (int)px + dx, sy = (int)py + dy;
        const uint32_t x = sx < 0 ? 0u : (sx >= (int)W ? W - 1u : (uint32_t)sx), y = sy < 0 ? 0u : (sy >= (int)H ? H - 1u : (uint32_t)sy);
        uint32_t clo, chi, wlo, whi;
        load_hdr(x, y, clo, chi);
        to_w_halves(clo, chi, wlo, whi);
        const rgb w = unpack_rgb(wlo, whi);
        const float d = load_depth(x, y);
        if (dy == -1 && dx == -1) { box_start(box, w); best = d; bx = x; by = y; }
        else { box_add(box, w); if (closer(d, best)) { best = d; bx = x; by = y; } }
        if (dy == 0 && dx == 0) cw = w;
    }
    uint32_t clo, chi;
    load_hdr(px, py, clo, chi);
    lo = clo; hi = chi;
    if (!haveHistory) return;
    const uint32_t mv = load_motion(bx, by);
    const Tap t = tap_of(px, py, half_value(mv & 0xFFFFu), half_value(mv >> 16), W, H);
    if (!t.inside) return;
    uint32_t a, b;
    load_history(t.x0, t.y0, a, b); const rgb t00 = unpack_rgb(a, b);
    load_history(t.x1, t.y0, a, b); const rgb t10 = unpack_rgb(a, b);
    load_history(t.x0, t.y1, a, b); const rgb t01 = unpack_rgb(a, b);
    load_history(t.x1, t.y1, a, b); const rgb t11 = unpack_rgb(a, b);
    const rgb h = tap_mix(t00, t10, t01, t11, t.fx, t.fy);
    if (!finite3(h)) return;
    resolve_words(h, cw, box, blend, chi >> 16, lo, hi);
}

// ---- jitter: the reference's Halton (MathUtils.cpp) and the DLSS branch of UpscalingManager::GetJitter, in fp32 ----------------------------------------------
BRMI_HD float halton(uint32_t i, uint32_t b) {
    float f = 1.0f, r = 0.0f;
    while (i > 0u) {
        f /= (float)b;
        r = r + f * (float)(i % b);
        i = (uint32_t)floorf((float)i / (float)b);
    }
    return r;
}
BRMI_HD void jitter_offset(uint32_t frameIndex, uint32_t phases, float& jx, float& jy) {
    const uint32_t i = frameIndex % phases;
    jx = halton(i + 1u, 2u) - 0.5f; jy = halton(i + 1u, 3u) - 0.5f;
}

}  // namespace temporal
}  // namespace brmi

#endif
