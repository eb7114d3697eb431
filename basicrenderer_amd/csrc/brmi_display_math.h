// brmi_display_math.h -- the display chain's arithmetic: luminance histogram bin and average, the LPM setup and mapper, the other tone curves, gamma, the
// UNORM store and the two bloom filters.  Plain C++ for host and device: brmi_display.hip's kernels and tests/display_main.cpp compile it.
//
// Restated from BR/shaders/PostProcessing/{luminanceHistogram, luminanceHistogramAverage, tonemapping, bloomDownsample, bloomUpsample, bloomBlend}.hlsl,
// BR/shaders/Include/gammaCorrection.hlsli and, for the one configuration the reference uses (shoulder 1, con 0, soft 0, con2 0, clip 1, scaleOnly 0; Rec.709
// with D65 as working, output and container space), LpmSetup / LpmMap of BR/shaders/FidelityFX/ffx_lpm.h.  Arithmetic: IEEE fp32 without contraction in the
// shader's order; a * b + c is two roundings; rcp(x) = 1 / x; saturate = min(max(x, 0), 1) through fmaxf / fminf, which return the other operand for a NaN
// (saturate(NaN) = 0, as in HLSL); log2, exp2 and pow are the math library's.
#ifndef BRMI_DISPLAY_MATH_H
#define BRMI_DISPLAY_MATH_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define BRMI_HD __host__ __device__ inline
#else
#define BRMI_HD inline
#endif

namespace brmi {
namespace display {

struct rgb { float r, g, b; };

constexpr float kMinLogLuminance = 0.001f;                   // the reference's MIN_LOG_LUMINANCE: not a logarithm, kept as it is
constexpr float kHdrMax = 10.0f, kSoftGap = 0.001f, kBloomRadius = 0.001f, kBloomBlend = 0.04f;
constexpr uint32_t kMaxBloomLevels = 5u, kMinBloomSide = 32u, kControlWords = 96u;
enum Curve : uint32_t { REINHARD_JODIE = 0u, KHRONOS_PBR_NEUTRAL = 1u, ACES_HILL = 2u, AMD_LPM = 3u, NONE = 4u };

BRMI_HD float dsat(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
BRMI_HD uint32_t bits_of(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
BRMI_HD float float_of(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
BRMI_HD float default_log_luminance_range() { return log2f(10.0f) - log2f(0.1f); }      // the reference's LOG_LUMINANCE_RANGE

// ---- halves: what an RGBA16F store keeps (round to nearest even; beyond 65520 infinity) ---------------------------------------------------------------
BRMI_HD uint32_t half_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)f);
#else
    const uint32_t u = bits_of(f), sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return sign | 0x7E00u;                        // NaN
    if (a >= 0x477FF000u) return sign | 0x7C00u;                       // rounds to infinity (65520 and up)
    if (a < 0x33000001u) return sign;                                  // rounds to zero (2^-25 and below)
    const int e = (int)(a >> 23) - 127;
    const uint32_t m = (a & 0x7FFFFFu) | 0x800000u;
    const int shift = e < -14 ? 13 + (-14 - e) : 13;                   // bits dropped from the 24-bit significand
    const uint32_t kept = m >> shift, rest = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
    uint32_t h = e < -14 ? kept : (((uint32_t)(e + 15) << 10) + (kept - 0x400u));
    if (rest > halfway || (rest == halfway && (h & 1u))) h++;          // (a carry runs into the exponent, which is the next binade)
    return sign | h;
#endif
}
BRMI_HD float half_value(uint32_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
#else
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 31u) return float_of(sign | 0x7F800000u | (m << 13));
    if (e == 0u) { const float v = (float)m * 5.9604644775390625e-8f; return sign ? -v : v; }      // m * 2^-24
    return float_of(sign | ((e + 112u) << 23) | (m << 13));
#endif
}
BRMI_HD float round_half(float f) { return half_value(half_bits(f)); }

// ---- LuminanceHistogramPass: colorToBin ---------------------------------------------------------------------------------------------------------------------
// A NaN luminance fails `< 0.005`, its logarithm saturates to 0: bin 1.  +inf: bin 255.  Negative: bin 0.
BRMI_HD uint32_t luminance_bin(float r, float g, float b, float minLog, float invRange) {
    const float lum = (r * 0.2125f + g * 0.7154f) + b * 0.0721f;
    if (lum < 0.005f) return 0u;
    const float logLum = dsat((log2f(lum) - minLog) * invRange);
    return (uint32_t)(logLum * 254.0f + 1.0f);
}
// ---- LuminanceHistogramAveragePass --------------------------------------------------------------------------------------------------------------------------
BRMI_HD uint32_t weighted_sum(const uint32_t counts[256]) {      // uint32, wrapping as the shader's LDS sum wraps
    uint32_t s = 0u;
    for (uint32_t i = 0; i < 256u; i++) s += counts[i] * i;
    return s;
}
BRMI_HD float average_luminance(uint32_t weightedSum, uint32_t count0, float numPixels, float minLog, float range) {
    const float weightedLogAverage = ((float)weightedSum / fmaxf(numPixels - (float)count0, 1.0f)) - 1.0f;
    return exp2f((weightedLogAverage / 254.0f) * range + minLog);
}
BRMI_HD float adapt_luminance(float last, float average, float timeCoefficient) { return last + (average - last) * timeCoefficient; }

// ---- LpmSetup -----------------------------------------------------------------------------------------------------------------------------------------------
struct LpmParams {      // what LpmMap reads of the control block in this configuration
    float saturation[3], contrast, toneScaleBias[2], lumaT[3], crosstalk[3], rcpLumaT[3], shoulderContrast;
};
BRMI_HD float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
BRMI_HD void xy_to_xyz(float d[3], const float s[2]) { d[0] = s[0]; d[1] = s[1]; d[2] = 1.0f - (s[0] + s[1]); }
BRMI_HD void mat_inv3(float ox[3], float oy[3], float oz[3], const float ix[3], const float iy[3], const float iz[3]) {
    const float i = 1.0f / ((ix[0] * (iy[1] * iz[2] - iz[1] * iy[2]) - ix[1] * (iy[0] * iz[2] - iy[2] * iz[0])) + ix[2] * (iy[0] * iz[1] - iy[1] * iz[0]));
    ox[0] = (iy[1] * iz[2] - iz[1] * iy[2]) * i; ox[1] = (ix[2] * iz[1] - ix[1] * iz[2]) * i; ox[2] = (ix[1] * iy[2] - ix[2] * iy[1]) * i;
    oy[0] = (iy[2] * iz[0] - iy[0] * iz[2]) * i; oy[1] = (ix[0] * iz[2] - ix[2] * iz[0]) * i; oy[2] = (iy[0] * ix[2] - ix[0] * iy[2]) * i;
    oz[0] = (iy[0] * iz[1] - iz[0] * iy[1]) * i; oz[1] = (iz[0] * ix[1] - ix[0] * iz[1]) * i; oz[2] = (ix[0] * iy[1] - iy[0] * ix[1]) * i;
}
// the Y row of the RGB -> XYZ matrix of a colour space given by its xy chromaticities, scaled to sum 1: the luma coefficients
BRMI_HD void luma_of_space(float luma[3], const float r[2], const float g[2], const float b[2], const float w[2]) {
    float rz[3], gz[3], bz[3];
    xy_to_xyz(rz, r); xy_to_xyz(gz, g); xy_to_xyz(bz, b);
    const float r3[3] = {rz[0], gz[0], bz[0]}, g3[3] = {rz[1], gz[1], bz[1]}, b3[3] = {rz[2], gz[2], bz[2]};      // the transpose
    float w3[3];
    xy_to_xyz(w3, w);
    const float rw = 1.0f / w[1];
    w3[0] = w3[0] * rw; w3[1] = w3[1] * rw; w3[2] = w3[2] * rw;
    float rv[3], gv[3], bv[3];
    mat_inv3(rv, gv, bv, r3, g3, b3);
    const float s[3] = {dot3(rv, w3), dot3(gv, w3), dot3(bv, w3)};
    const float y[3] = {g3[0] * s[0], g3[1] * s[1], g3[2] * s[2]};
    const float rs = 1.0f / ((y[0] + y[1]) + y[2]);
    luma[0] = y[0] * rs; luma[1] = y[1] * rs; luma[2] = y[2] * rs;
}
BRMI_HD float exposure_of(float adaptedLuminance) { return log2f(kHdrMax * 0.18f / fmaxf(adaptedLuminance, 1e-5f)); }
BRMI_HD LpmParams lpm_params(float adaptedLuminance) {
    LpmParams p;
    const float exposure = exposure_of(adaptedLuminance);
    const float contrast = 0.0f + 1.0f, shoulderContrast = 1.0f, hdrMax = kHdrMax;
    p.saturation[0] = p.saturation[1] = p.saturation[2] = 0.0f + contrast;
    p.contrast = contrast; p.shoulderContrast = shoulderContrast;
    p.crosstalk[0] = p.crosstalk[1] = p.crosstalk[2] = 1.0f;
    const float midIn = (hdrMax * 0.18f) * exp2f(-exposure), midOut = 0.18f;
    const float cs = contrast * shoulderContrast;
    const float z0 = -powf(midIn, contrast);
    const float z1 = powf(hdrMax, cs) * powf(midIn, contrast);
    const float z2 = (powf(hdrMax, contrast) * powf(midIn, cs)) * midOut;
    const float z3 = powf(hdrMax, cs) * midOut;
    const float z4 = powf(midIn, cs) * midOut;
    p.toneScaleBias[0] = -((z0 + (midOut * (z1 - z2)) * (1.0f / (z3 - z4))) * (1.0f / z4));
    p.toneScaleBias[1] = (z1 - z2) * (1.0f / (z3 - z4));      // (w0 .. w3 of the text are z1 .. z4 again)
    const float R[2] = {0.64f, 0.33f}, G[2] = {0.30f, 0.60f}, B[2] = {0.15f, 0.06f}, D65[2] = {0.3127f, 0.3290f};
    luma_of_space(p.lumaT, R, G, B, D65);      // soft 0: lumaT is the working space's, which is lumaW
    p.rcpLumaT[0] = 1.0f / p.lumaT[0]; p.rcpLumaT[1] = 1.0f / p.lumaT[1]; p.rcpLumaT[2] = 1.0f / p.lumaT[2];
    return p;
}
// the 24 x 4-word control block in the reference's packing: the fp32 words; the packed-half words (16-20) and the reserved ones stay zero
BRMI_HD void lpm_pack(const LpmParams& p, uint32_t ctl[96]) {
    for (uint32_t i = 0; i < kControlWords; i++) ctl[i] = 0u;
    ctl[0] = bits_of(p.saturation[0]); ctl[1] = bits_of(p.saturation[1]); ctl[2] = bits_of(p.saturation[2]); ctl[3] = bits_of(p.contrast);
    ctl[4] = bits_of(p.toneScaleBias[0]); ctl[5] = bits_of(p.toneScaleBias[1]); ctl[6] = bits_of(p.lumaT[0]); ctl[7] = bits_of(p.lumaT[1]);
    ctl[8] = bits_of(p.lumaT[2]); ctl[9] = bits_of(p.crosstalk[0]); ctl[10] = bits_of(p.crosstalk[1]); ctl[11] = bits_of(p.crosstalk[2]);
    ctl[12] = bits_of(p.rcpLumaT[0]); ctl[13] = bits_of(p.rcpLumaT[1]); ctl[14] = bits_of(p.rcpLumaT[2]);      // 15 - 23: con2R/G/B = 0
    ctl[24] = bits_of(p.shoulderContrast); ctl[25] = bits_of(p.lumaT[0]); ctl[26] = bits_of(p.lumaT[1]); ctl[27] = bits_of(p.lumaT[2]);      // lumaW
    // 28 - 38: softGap and conR/G/B = 0 (soft 0, con 0)
}
BRMI_HD LpmParams lpm_unpack(const uint32_t* ctl) {
    LpmParams p;
    p.saturation[0] = float_of(ctl[0]); p.saturation[1] = float_of(ctl[1]); p.saturation[2] = float_of(ctl[2]); p.contrast = float_of(ctl[3]);
    p.toneScaleBias[0] = float_of(ctl[4]); p.toneScaleBias[1] = float_of(ctl[5]); p.lumaT[0] = float_of(ctl[6]); p.lumaT[1] = float_of(ctl[7]);
    p.lumaT[2] = float_of(ctl[8]); p.crosstalk[0] = float_of(ctl[9]); p.crosstalk[1] = float_of(ctl[10]); p.crosstalk[2] = float_of(ctl[11]);
    p.rcpLumaT[0] = float_of(ctl[12]); p.rcpLumaT[1] = float_of(ctl[13]); p.rcpLumaT[2] = float_of(ctl[14]); p.shoulderContrast = float_of(ctl[24]);
    return p;
}
BRMI_HD void lpm_setup(float adaptedLuminance, uint32_t ctl[96]) { lpm_pack(lpm_params(adaptedLuminance), ctl); }

// ---- LpmMap (shoulder 1, con 0, soft 0, con2 0).  A black pixel: rcp(0) * 0 = NaN in the ratios, which the saturates turn into 0. --------------------------------
BRMI_HD rgb lpm_map(rgb c, const LpmParams& p) {
    const float rcpMax = 1.0f / fmaxf(fmaxf(c.r, c.g), c.b);
    float ratioR = c.r * rcpMax, ratioG = c.g * rcpMax, ratioB = c.b * rcpMax;
    ratioR = powf(ratioR, p.saturation[0]); ratioG = powf(ratioG, p.saturation[1]); ratioB = powf(ratioB, p.saturation[2]);
    float luma = c.g * p.lumaT[1] + (c.r * p.lumaT[0] + (c.b * p.lumaT[2]));
    luma = powf(luma, p.contrast);
    const float lumaShoulder = powf(luma, p.shoulderContrast);
    luma = luma * (1.0f / (lumaShoulder * p.toneScaleBias[0] + p.toneScaleBias[1]));
    const float lumaRatio = (ratioR * p.lumaT[0] + ratioG * p.lumaT[1]) + ratioB * p.lumaT[2];
    const float ratioScale = dsat(luma * (1.0f / lumaRatio));
    float colorR = dsat(ratioR * ratioScale), colorG = dsat(ratioG * ratioScale), colorB = dsat(ratioB * ratioScale);
    const float capR = -p.crosstalk[0] * colorR + p.crosstalk[0], capG = -p.crosstalk[1] * colorG + p.crosstalk[1], capB = -p.crosstalk[2] * colorB + p.crosstalk[2];
    float lumaAdd = dsat((-colorB) * p.lumaT[2] + ((-colorR) * p.lumaT[0] + ((-colorG) * p.lumaT[1] + luma)));
    const float t = lumaAdd * (1.0f / (capG * p.lumaT[1] + (capR * p.lumaT[0] + (capB * p.lumaT[2]))));
    colorR = dsat(t * capR + colorR); colorG = dsat(t * capG + colorG); colorB = dsat(t * capB + colorB);
    lumaAdd = dsat((-colorB) * p.lumaT[2] + ((-colorR) * p.lumaT[0] + ((-colorG) * p.lumaT[1] + luma)));
    colorR = dsat(lumaAdd * p.rcpLumaT[0] + colorR); colorG = dsat(lumaAdd * p.rcpLumaT[1] + colorG); colorB = dsat(lumaAdd * p.rcpLumaT[2] + colorB);
    return rgb{colorR, colorG, colorB};
}

// ---- tonemapping.hlsl ----------------------------------------------------------------------------------------------------------------------------------------
BRMI_HD rgb reinhard_jodie(rgb c) {
    const float luminance = (c.r * 0.2126f + c.g * 0.7152f) + c.b * 0.0722f;
    const rgb pc{c.r / (1.0f + c.r), c.g / (1.0f + c.g), c.b / (1.0f + c.b)};
    const rgb lm{c.r / (1.0f + luminance), c.g / (1.0f + luminance), c.b / (1.0f + luminance)};
    return rgb{lm.r + pc.r * (pc.r - lm.r), lm.g + pc.g * (pc.g - lm.g), lm.b + pc.b * (pc.b - lm.b)};      // lerp(lm, pc, pc)
}
BRMI_HD rgb khronos_pbr_neutral(rgb c) {
    const float startCompression = 0.8f - 0.04f, desaturation = 0.15f;
    const float x = fminf(c.r, fminf(c.g, c.b));
    const float offset = x < 0.08f ? x - (6.25f * x) * x : 0.04f;
    c.r -= offset; c.g -= offset; c.b -= offset;
    const float peak = fmaxf(c.r, fmaxf(c.g, c.b));
    if (peak < startCompression) return c;
    const float d = 1.0f - startCompression;
    const float newPeak = 1.0f - (d * d) / ((peak + d) - startCompression);
    const float scale = newPeak / peak;
    c.r *= scale; c.g *= scale; c.b *= scale;
    const float g = 1.0f - 1.0f / (desaturation * (peak - newPeak) + 1.0f);
    return rgb{c.r + g * (newPeak - c.r), c.g + g * (newPeak - c.g), c.b + g * (newPeak - c.b)};
}
BRMI_HD float rrt_and_odt_fit(float v) {
    const float a = v * (v + 0.0245786f) - 0.000090537f, b = v * (0.983729f * v + 0.4329510f) + 0.238081f;
    return a / b;
}
BRMI_HD rgb aces_hill(rgb c) {      // mul(color, M): the row vector times the matrix as its rows are written
    rgb v{(c.r * 0.59719f + c.g * 0.35458f) + c.b * 0.04823f, (c.r * 0.07600f + c.g * 0.90834f) + c.b * 0.01566f, (c.r * 0.02840f + c.g * 0.13383f) + c.b * 0.83777f};
    v = rgb{rrt_and_odt_fit(v.r), rrt_and_odt_fit(v.g), rrt_and_odt_fit(v.b)};
    const rgb o{(v.r * 1.60475f + v.g * -0.53108f) + v.b * -0.07367f, (v.r * -0.10208f + v.g * 1.10813f) + v.b * -0.00605f, (v.r * -0.00327f + v.g * -0.07276f) + v.b * 1.07602f};
    return rgb{dsat(o.r), dsat(o.g), dsat(o.b)};
}
template <uint32_t CURVE> BRMI_HD rgb tone_map(rgb c, const LpmParams& lpm) {
    if (CURVE == REINHARD_JODIE) return reinhard_jodie(c);
    if (CURVE == KHRONOS_PBR_NEUTRAL) return khronos_pbr_neutral(c);
    if (CURVE == ACES_HILL) return aces_hill(c);
    if (CURVE == AMD_LPM) return lpm_map(c, lpm);
    return c;      // the switch's default: no tone mapping
}
BRMI_HD rgb tone_map_of(uint32_t curve, rgb c, const LpmParams& lpm) {
    switch (curve) {
        case REINHARD_JODIE: return tone_map<REINHARD_JODIE>(c, lpm);
        case KHRONOS_PBR_NEUTRAL: return tone_map<KHRONOS_PBR_NEUTRAL>(c, lpm);
        case ACES_HILL: return tone_map<ACES_HILL>(c, lpm);
        case AMD_LPM: return tone_map<AMD_LPM>(c, lpm);
        default: return c;
    }
}
// gammaCorrection.hlsli's LinearToSRGB: a power, not the sRGB curve.  A negative base gives NaN, which the store below writes as 0.
BRMI_HD float gamma_correct(float x) { return powf(x, 1.0f / 2.2f); }
BRMI_HD uint32_t unorm8_code(float x) { return (uint32_t)(dsat(x) * 255.0f + 0.5f); }
BRMI_HD uint32_t ldr_pixel(rgb mapped) {      // R8G8B8A8_UNORM with alpha 1
    return unorm8_code(gamma_correct(mapped.r)) | (unorm8_code(gamma_correct(mapped.g)) << 8) | (unorm8_code(gamma_correct(mapped.b)) << 16) | 0xFF000000u;
}

// ---- bloom ---------------------------------------------------------------------------------------------------------------------------------------------------------
BRMI_HD uint32_t bloom_level_count(uint32_t W, uint32_t H) {      // min(5, floor(log2(max(W, H))) + 1)
    uint32_t n = 0u;
    for (uint32_t m = W > H ? W : H; m; m >>= 1) n++;
    return n < kMaxBloomLevels ? n : kMaxBloomLevels;
}
BRMI_HD bool bloom_possible(uint32_t W, uint32_t H) { return (W < H ? W : H) >= kMinBloomSide; }      // below, a level has no rows: the reference draws nothing there
BRMI_HD uint32_t bloom_level_size(uint32_t size, uint32_t level) { return size >> level; }

// SampleLevel(g_linearClamp, uv, 0): the four texels and the two weights (fp32 weights, clamped texel coordinates)
struct Bilinear { uint32_t x0, x1, y0, y1; float fx, fy; };
BRMI_HD uint32_t clamp_texel(float f, uint32_t n) {
    const float hi = (float)(n - 1u);
    const float c = fminf(fmaxf(f, 0.0f), hi);
    return (uint32_t)c;
}
BRMI_HD Bilinear bilinear_of(float u, float v, uint32_t W, uint32_t H) {
    Bilinear b;
    const float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    const float x0f = floorf(x), y0f = floorf(y);
    b.fx = x - x0f; b.fy = y - y0f;
    b.x0 = clamp_texel(x0f, W); b.x1 = clamp_texel(x0f + 1.0f, W); b.y0 = clamp_texel(y0f, H); b.y1 = clamp_texel(y0f + 1.0f, H);
    return b;
}
BRMI_HD float bilinear_mix(float t00, float t10, float t01, float t11, float fx, float fy) {
    const float r0 = t00 + fx * (t10 - t00), r1 = t01 + fx * (t11 - t01);
    return r0 + fy * (r1 - r0);
}
// the 13 taps of bloomDownsample.hlsl in the text's letters a .. m: offsets in units of the source texel size (x, y)
BRMI_HD void bloom_down_offset(int k, float& ox, float& oy) {
    const float X[13] = {-2.0f, 0.0f, 2.0f, -2.0f, 0.0f, 2.0f, -2.0f, 0.0f, 2.0f, -1.0f, 1.0f, -1.0f, 1.0f};
    const float Y[13] = {2.0f, 2.0f, 2.0f, 0.0f, 0.0f, 0.0f, -2.0f, -2.0f, -2.0f, 1.0f, 1.0f, -1.0f, -1.0f};
    ox = X[k]; oy = Y[k];
}
BRMI_HD float bloom_down_combine(const float t[13]) {      // one channel
    float d = t[4] * 0.125f;
    d += (((t[0] + t[2]) + t[6]) + t[8]) * 0.03125f;
    d += (((t[1] + t[3]) + t[5]) + t[7]) * 0.0625f;
    d += (((t[9] + t[10]) + t[11]) + t[12]) * 0.125f;
    return d;
}
// max(v, 1e-5), then length(v) < 1 writes (0, 0, 0, 1); returns whether the texel is kept
BRMI_HD bool bloom_down_tail(rgb& v) {
    v.r = fmaxf(v.r, 0.00001f); v.g = fmaxf(v.g, 0.00001f); v.b = fmaxf(v.b, 0.00001f);
    const float len = sqrtf((v.r * v.r + v.g * v.g) + v.b * v.b);
    if (len < 1.0f) { v = rgb{0.0f, 0.0f, 0.0f}; return false; }
    return true;
}
// the 9 taps of sample_for_upsample, a .. i: offsets in units of (x, y) = (radius, radius * aspect)
BRMI_HD void bloom_tent_offset(int k, float& ox, float& oy) {
    const float X[9] = {-1.0f, 0.0f, 1.0f, -1.0f, 0.0f, 1.0f, -1.0f, 0.0f, 1.0f};
    const float Y[9] = {1.0f, 1.0f, 1.0f, 0.0f, 0.0f, 0.0f, -1.0f, -1.0f, -1.0f};
    ox = X[k]; oy = Y[k];
}
BRMI_HD float bloom_tent_combine(const float t[9]) {
    float u = t[4] * 4.0f;
    u += (((t[1] + t[3]) + t[5]) + t[7]) * 2.0f;
    u += ((t[0] + t[2]) + t[6]) + t[8];
    u *= 1.0f / 16.0f;
    return u;
}
BRMI_HD float bloom_add(float dst, float tent) { return round_half(dst + tent); }                                   // the additive blend into an RGBA16F level
BRMI_HD float bloom_blend(float existing, float bloom) { return round_half(existing + kBloomBlend * (bloom - existing)); }      // lerp(existing, bloom, 0.04), stored

}  // namespace display
}  // namespace brmi
#endif
