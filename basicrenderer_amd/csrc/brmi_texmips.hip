// brmi_texmips.hip -- mip chains of material textures for gfx950: the plain chain and the alpha-coverage chain.
//
// Reference: BR/shaders/Utilities/mipmapping.hlsl over BR/shaders/FidelityFX/ffx_spd.h (Float4, non-array MipmapCSMain),
// BR/shaders/Utilities/alphaCoverageMipmapping.hlsl, the job loop of BR/src/Factories/TextureFactory.cpp:1040-1300.
// The bytes are the contract (tests/texmips_ref.py restates them); what differs is how the work is laid on the machine:
//   * plain chain, ONE launch: a workgroup of 256 threads owns a 64 x 64 source tile and carries levels 1..6 of it in registers and LDS as unquantised fp32, in
//     SPD's operand order (levels 1 and 7 add (0,0) (0,1) (1,0) (1,1), the quad levels (0,0) (1,0) (0,1) (1,1)).  A 2 x 2 quad is four neighbouring lanes, so a
//     quad level is three DPP quad_perm moves, no LDS round trip.  The last workgroup to finish (an ordinary device atomic behind a fence) re-reads the STORED
//     level 6 and builds levels 7.. the same way, and leaves the counter at zero for the next build;
//   * alpha chain, per level two launches (statistics are needed before the scale): downsample + statistics, then resolve + apply.  The 256-bin histogram and the
//     three counts are LDS counters of a workgroup, flushed once per bin (integers: the sums do not depend on the order); the serial scan from bin 255 down is
//     done by one lane of every workgroup of the apply launch from an LDS copy of the 260 words (255 dependent LDS reads instead of a launch of one thread);
//     the reset of all levels' words is one launch in front.
// Arithmetic: IEEE fp32, no contraction.  A texel code decodes through the tables of brmi_texture.h (code / 255.0f; rgb of an sRGB texture through the scene's
// 256-entry table).  The sRGB encode is LinearToSrgb of the shader text with the device library's powf; the store is (uint)(saturate(x) * 255 + 0.5).
#include <algorithm>

#include "brmi_internal.h"
#include "brmi_texture.h"

namespace brmi {

constexpr uint32_t kStatsWords = 260u, kPrevCovered = 0u, kPrevTotal = 1u, kDstTotal = 2u, kHistBase = 3u;

BRMI_DEV f4 operator+(f4 a, f4 b) { return {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
BRMI_DEV f4 reduce4(f4 v0, f4 v1, f4 v2, f4 v3) { const f4 s = ((v0 + v1) + v2) + v3; return {s.x * 0.25f, s.y * 0.25f, s.z * 0.25f, s.w * 0.25f}; }
// LinearToSrgb of both shaders: lerp(lo, hi, step(0.0031308f, c)) = lo + s * (hi - lo)
BRMI_DEV float linear_to_srgb(float c) {
    c = sat(c);
    const float lo = c * 12.92f, hi = 1.055f * powf(c, 1.0f / 2.4f) - 0.055f;
    const float useHi = c >= 0.0031308f ? 1.0f : 0.0f;
    return lo + useHi * (hi - lo);
}
BRMI_DEV uint32_t encode_texel(f4 v, bool srgb) {
    if (srgb) { v.x = linear_to_srgb(v.x); v.y = linear_to_srgb(v.y); v.z = linear_to_srgb(v.z); }
    return pack_unorm4(v.x, v.y, v.z, v.w);
}
BRMI_DEV f4 decode_texel(const float* tables, uint32_t t, bool srgb) {
    const float* rgb = tables + (srgb ? 256u : 0u);
    return {rgb[t & 0xFFu], rgb[(t >> 8) & 0xFFu], rgb[(t >> 16) & 0xFFu], tables[t >> 24]};
}
BRMI_DEV uint32_t level_dim(uint32_t d, uint32_t l) { return d >> l ? d >> l : 1u; }

// ================================================ the plain chain (SPD) ================================================
struct SpdArgs {
    uint32_t* texels; const float* srgbToLinear; uint32_t* counter;
    uint32_t width, height, levels /* mipCount */, srgb, groupsX, groups;
    uint32_t offset[13];
};
// a value of lane quad|k in every lane of the quad (DPP quad_perm [k, k, k, k])
template <int K> BRMI_DEV float quad_read(float v) { return as_f32((uint32_t)__builtin_amdgcn_update_dpp(0, (int)as_u32(v), K * 0x55, 0xF, 0xF, false)); }
template <int K> BRMI_DEV f4 quad_read4(f4 v) { return {quad_read<K>(v.x), quad_read<K>(v.y), quad_read<K>(v.z), quad_read<K>(v.w)}; }
BRMI_DEV f4 reduce_quad(f4 v) { return reduce4(v, quad_read4<1>(v), quad_read4<2>(v), quad_read4<3>(v)); }      // what lane quad|0 keeps

struct SpdCtx {
    const SpdArgs& a; const float* tables; float (*inter)[16][16];      // inter[channel][x][y]
    BRMI_DEV f4 load_source(uint32_t x, uint32_t y) const {
        x = x < a.width - 1u ? x : a.width - 1u; y = y < a.height - 1u ? y : a.height - 1u;
        return decode_texel(tables, a.texels[(size_t)y * a.width + x], a.srgb != 0u);
    }
    BRMI_DEV f4 reduce_source(uint32_t x, uint32_t y) const { return reduce4(load_source(x, y), load_source(x, y + 1u), load_source(x + 1u, y), load_source(x + 1u, y + 1u)); }
    // SpdLoad: the stored level 6 as stored (no decode), clamped to the level
    BRMI_DEV f4 load_stored6(uint32_t x, uint32_t y) const {
        const uint32_t w = level_dim(a.width, 6u), h = level_dim(a.height, 6u);
        x = x < w - 1u ? x : w - 1u; y = y < h - 1u ? y : h - 1u;
        return decode_texel(tables, a.texels[(size_t)a.offset[6] + (size_t)y * w + x], false);
    }
    BRMI_DEV f4 reduce_stored6(uint32_t x, uint32_t y) const { return reduce4(load_stored6(x, y), load_stored6(x, y + 1u), load_stored6(x + 1u, y), load_stored6(x + 1u, y + 1u)); }
    BRMI_DEV void store(uint32_t level, uint32_t x, uint32_t y, f4 v) const {
        const uint32_t w = level_dim(a.width, level), h = level_dim(a.height, level);
        if (level >= a.levels || x >= w || y >= h) return;
        a.texels[(size_t)a.offset[level] + (size_t)y * w + x] = encode_texel(v, a.srgb != 0u);
    }
    BRMI_DEV f4 load_inter(uint32_t x, uint32_t y) const { return {inter[0][x][y], inter[1][x][y], inter[2][x][y], inter[3][x][y]}; }
    BRMI_DEV void store_inter(uint32_t x, uint32_t y, f4 v) const { inter[0][x][y] = v.x; inter[1][x][y] = v.y; inter[2][x][y] = v.z; inter[3][x][y] = v.w; }
    // SpdDownsampleNextFour: four quad levels from the 16 x 16 intermediates; `level` is the first of them, (gx, gy) the workgroup's tile
    BRMI_DEV void next_four(uint32_t x, uint32_t y, uint32_t gx, uint32_t gy, uint32_t tid, uint32_t level) const {
        if (a.levels <= level) return;
        __syncthreads();
        {
            const f4 v = reduce_quad(load_inter(x, y));
            if ((tid & 3u) == 0u) { store(level, gx * 8u + x / 2u, gy * 8u + y / 2u, v); store_inter(x + (y / 2u) % 2u, y, v); }
        }
        if (a.levels <= level + 1u) return;
        __syncthreads();
        if (tid < 64u) {
            const f4 v = reduce_quad(load_inter(x * 2u + y % 2u, y * 2u));
            if ((tid & 3u) == 0u) { store(level + 1u, gx * 4u + x / 2u, gy * 4u + y / 2u, v); store_inter(x * 2u + y / 2u, y * 2u, v); }
        }
        if (a.levels <= level + 2u) return;
        __syncthreads();
        if (tid < 16u) {
            const f4 v = reduce_quad(load_inter(x * 4u + y, y * 4u));
            if ((tid & 3u) == 0u) { store(level + 2u, gx * 2u + x / 2u, gy * 2u + y / 2u, v); store_inter(x / 2u + y, 0u, v); }
        }
        if (a.levels <= level + 3u) return;
        __syncthreads();
        if (tid < 4u) {
            const f4 v = reduce_quad(load_inter(tid, 0u));
            if ((tid & 3u) == 0u) store(level + 3u, gx, gy, v);
        }
    }
};

__global__ void __launch_bounds__(256) k_texmips_spd(SpdArgs a) {
    __shared__ float tables[512];
    __shared__ float inter[4][16][16];
    __shared__ uint32_t ticket;
    const uint32_t tid = threadIdx.x;
    stage_texel_tables(tables, a.srgbToLinear, tid, 256u);
    __syncthreads();
    const SpdCtx c{a, tables, inter};
    const uint32_t gx = blockIdx.x % a.groupsX, gy = blockIdx.x / a.groupsX;
    // ARmpRed8x8: lanes 0..3 of a quad are (0,0) (1,0) (0,1) (1,1); a wave is an 8 x 8 block of the 16 x 16 threads
    const uint32_t l6 = tid & 63u;
    const uint32_t x = ((((l6 >> 2) & 7u) & ~1u) | (l6 & 1u)) + 8u * ((tid >> 6) & 1u);
    const uint32_t y = ((((l6 >> 3) & 7u) & ~3u) | ((l6 >> 1) & 3u)) + 8u * (tid >> 7);
    {   // SpdDownsampleMips_0_1: levels 1 and 2
        f4 v[4];
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            const uint32_t ox = (i & 1u) * 16u, oy = (i >> 1) * 16u;
            v[i] = c.reduce_source(gx * 64u + (x + ox) * 2u, gy * 64u + (y + oy) * 2u);
            c.store(1u, gx * 32u + x + ox, gy * 32u + y + oy, v[i]);
        }
        if (a.levels <= 2u) return;
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            v[i] = reduce_quad(v[i]);
            if ((tid & 3u) == 0u) {
                const uint32_t ox = (i & 1u) * 8u, oy = (i >> 1) * 8u;
                c.store(2u, gx * 16u + x / 2u + ox, gy * 16u + y / 2u + oy, v[i]);
                c.store_inter(x / 2u + ox, y / 2u + oy, v[i]);
            }
        }
    }
    c.next_four(x, y, gx, gy, tid, 3u);      // levels 3..6
    if (a.levels <= 7u) return;
    // SpdExitWorkgroup: this workgroup's stores of level 6 are released, then the ticket is taken; only the last one goes on
    __threadfence();
    __syncthreads();
    if (tid == 0u) ticket = atomicAdd(a.counter, 1u);
    __syncthreads();
    if (ticket != a.groups - 1u) return;
    __threadfence();
    if (tid == 0u) *a.counter = 0u;
    {   // SpdDownsampleMips_6_7: levels 7 and 8 from the stored level 6
        f4 v[4];
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            const uint32_t ox = i & 1u, oy = i >> 1;
            v[i] = c.reduce_stored6(x * 4u + ox * 2u, y * 4u + oy * 2u);
            c.store(7u, x * 2u + ox, y * 2u + oy, v[i]);
        }
        if (a.levels <= 8u) return;
        const f4 r = reduce4(v[0], v[1], v[2], v[3]);
        c.store(8u, x, y, r);
        c.store_inter(x, y, r);
    }
    c.next_four(x, y, 0u, 0u, tid, 9u);      // levels 9..12
}

// ================================================ the alpha-coverage chain ================================================
struct AlphaArgs {
    uint32_t* texels; const float* srgbToLinear; uint32_t* stats /* this level's 260 words */; float* scale /* this level's */;
    uint32_t srcOffset, dstOffset, srcW, srcH, dstW, dstH, srgb;
};
__global__ void __launch_bounds__(256) k_alpha_reset(uint32_t* stats, float* scales, uint32_t levels) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < (levels - 1u) * kStatsWords) stats[kStatsWords + i] = 0u;
    if (i >= 1u && i < levels) scales[i] = 1.0f;
}
BRMI_DEV f4 alpha_load(const AlphaArgs& a, const float* tables, int x, int y) {      // clamped to the source level
    x = x < 0 ? 0 : (x > (int)a.srcW - 1 ? (int)a.srcW - 1 : x); y = y < 0 ? 0 : (y > (int)a.srcH - 1 ? (int)a.srcH - 1 : y);
    return decode_texel(tables, a.texels[(size_t)a.srcOffset + (size_t)y * a.srcW + x], a.srgb != 0u);
}
__global__ void __launch_bounds__(256) k_alpha_downsample(AlphaArgs a) {
    __shared__ float tables[512];
    __shared__ uint32_t local[kStatsWords];
    const uint32_t tid = threadIdx.x;
    stage_texel_tables(tables, a.srgbToLinear, tid, 256u);
    local[tid] = 0u; if (tid < kStatsWords - 256u) local[256u + tid] = 0u;
    __syncthreads();
    const uint32_t w = tid >> 6, lane = tid & 63u;      // a wave is an 8 x 8 quarter of the workgroup's 16 x 16 destination tile
    const uint32_t dx = blockIdx.x * 16u + (w & 1u) * 8u + (lane & 7u), dy = blockIdx.y * 16u + (w >> 1) * 8u + (lane >> 3);
    if (dx < a.dstW && dy < a.dstH) {
        f3 rgbSum{0.0f, 0.0f, 0.0f};
        float alphaSum = 0.0f;
        uint32_t total = 0u, covered = 0u;
#pragma nounroll
        for (uint32_t k = 0; k < 4u; k++) {
            const int sx = (int)(dx * 2u + (k & 1u)), sy = (int)(dy * 2u + (k >> 1));
            const f4 center = alpha_load(a, tables, sx, sy);
            f3 rgb{center.x, center.y, center.z};
            if (!(center.w >= 0.5f)) {      // DilatedRgb: the first texel of the 5 x 5 block at or over the cutoff, else the most opaque one
                float bestAlpha = center.w;
                bool found = false;
#pragma nounroll
                for (int j = 0; j < 25 && !found; j++) {
                    const f4 s = alpha_load(a, tables, sx + j % 5 - 2, sy + j / 5 - 2);
                    if (s.w > bestAlpha) { bestAlpha = s.w; rgb = f3{s.x, s.y, s.z}; }
                    if (s.w >= 0.5f) { rgb = f3{s.x, s.y, s.z}; found = true; }
                }
            }
            rgbSum = rgbSum + rgb;
            alphaSum = alphaSum + center.w;
            if ((uint32_t)sx < a.srcW && (uint32_t)sy < a.srcH) { total++; if (center.w >= 0.5f) covered++; }
        }
        const f4 out{rgbSum.x * 0.25f, rgbSum.y * 0.25f, rgbSum.z * 0.25f, alphaSum * 0.25f};
        a.texels[(size_t)a.dstOffset + (size_t)dy * a.dstW + dx] = encode_texel(out, a.srgb != 0u);
        const uint32_t bin = min(255u, (uint32_t)rintf(sat(out.w) * 255.0f));      // HLSL round: half to even
        atomicAdd(&local[kHistBase + bin], 1u);
        atomicAdd(&local[kDstTotal], 1u);
        if (total) atomicAdd(&local[kPrevTotal], total);
        if (covered) atomicAdd(&local[kPrevCovered], covered);
    }
    __syncthreads();
    for (uint32_t i = tid; i < kStatsWords; i += 256u) { const uint32_t v = local[i]; if (v) atomicAdd(a.stats + i, v); }
}
__global__ void __launch_bounds__(256) k_alpha_apply(AlphaArgs a) {
    __shared__ uint32_t local[kStatsWords];
    __shared__ float scaleShared;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kStatsWords; i += 256u) local[i] = a.stats[i];
    __syncthreads();
    if (tid == 0u) {      // AlphaMipResolveScaleCS
        const uint32_t prevTotal = local[kPrevTotal], prevCovered = local[kPrevCovered], dstTotal = local[kDstTotal];
        float scale = 1.0f;
        if (prevTotal != 0u && dstTotal != 0u && prevCovered != 0u) {
            const float targetCoverage = (float)prevCovered / (float)prevTotal;
            const uint32_t targetCovered = min(dstTotal, max(1u, (uint32_t)rintf(targetCoverage * (float)dstTotal)));
            uint32_t accumulated = 0u, selectedBin = 255u;
            for (int bin = 255; bin >= 1; --bin) {
                accumulated += local[kHistBase + (uint32_t)bin];
                if (accumulated >= targetCovered) { selectedBin = (uint32_t)bin; break; }
            }
            const float selectedAlpha = max2((float)selectedBin / 255.0f, 1.0f / 255.0f);
            scale = clampf(0.55f / selectedAlpha, 0.25f, 16.0f);
        }
        scaleShared = scale;
        if (blockIdx.x == 0u && blockIdx.y == 0u) *a.scale = scale;
    }
    __syncthreads();
    const float scale = scaleShared;
    const uint32_t w = tid >> 6, lane = tid & 63u;
    const uint32_t dx = blockIdx.x * 16u + (w & 1u) * 8u + (lane & 7u), dy = blockIdx.y * 16u + (w >> 1) * 8u + (lane >> 3);
    if (dx >= a.dstW || dy >= a.dstH) return;
    uint32_t* p = a.texels + (size_t)a.dstOffset + (size_t)dy * a.dstW + dx;
    const uint32_t t = *p;
    *p = (t & 0x00FFFFFFu) | (unorm8(sat(unorm8_to_f32(t >> 24) * scale)) << 24);      // rgb codes store back as they are
}

static int launched() { return hipGetLastError() == hipSuccess ? BRMI_OK : BRMI_ERR_HIP; }
int launch_texmips_plain(const brmi_texture_desc& d, const float* srgbToLinear, uint32_t* counter, hipStream_t s) {
    SpdArgs a{};
    a.texels = reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(d.texels)); a.srgbToLinear = srgbToLinear; a.counter = counter;
    a.width = d.width; a.height = d.height; a.levels = d.mipCount; a.srgb = d.format == BRMI_TEXTURE_FORMAT_RGBA8_UNORM_SRGB ? 1u : 0u;
    a.groupsX = (d.width + 63u) / 64u; a.groups = a.groupsX * ((d.height + 63u) / 64u);
    for (uint32_t l = 0; l < d.mipCount && l < 13u; l++) a.offset[l] = d.mipOffset[l];
    hipLaunchKernelGGL(k_texmips_spd, dim3(a.groups), dim3(256), 0, s, a);
    return launched();
}
int launch_texmips_alpha(const brmi_texture_desc& d, const float* srgbToLinear, uint32_t* stats, float* scales, hipStream_t s) {
    hipLaunchKernelGGL(k_alpha_reset, dim3(((d.mipCount - 1u) * kStatsWords + 255u) / 256u), dim3(256), 0, s, stats, scales, d.mipCount);
    for (uint32_t l = 1; l < d.mipCount; l++) {
        AlphaArgs a{};
        a.texels = reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(d.texels)); a.srgbToLinear = srgbToLinear;
        a.stats = stats + (size_t)l * kStatsWords; a.scale = scales + l;
        a.srcOffset = d.mipOffset[l - 1u]; a.dstOffset = d.mipOffset[l];
        a.srcW = std::max(1u, d.width >> (l - 1u)); a.srcH = std::max(1u, d.height >> (l - 1u));
        a.dstW = std::max(1u, d.width >> l); a.dstH = std::max(1u, d.height >> l);
        a.srgb = d.format == BRMI_TEXTURE_FORMAT_RGBA8_UNORM_SRGB ? 1u : 0u;
        const dim3 grid((a.dstW + 15u) / 16u, (a.dstH + 15u) / 16u);
        hipLaunchKernelGGL(k_alpha_downsample, grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_alpha_apply, grid, dim3(256), 0, s, a);
    }
    return launched();
}

}  // namespace brmi
