// brmi_display.hip -- the display chain for gfx950: luminance histogram and average (auto-exposure), the bloom pyramid, tone mapping into RGBA8.
//
// Restates the reference's LuminanceHistogramPass, LuminanceHistogramAveragePass, BuildBloomPipeline (five downsamples, four additive upsamples, the blend) and
// TonemappingPass; the arithmetic is brmi_display_math.h's, shared with the host.  MI355X-first differences:
//   * the full-screen pixel-shader passes are compute passes over the surfaces' tiled 8x8 layout: one wave is one tile, its loads and stores one contiguous run;
//   * the histogram is built per workgroup in LDS (a wave whose 64 pixels share a bin adds once), then one global atomic per non-empty bin and workgroup;
//   * the first downsample reads the pass's HDR target itself, and the blend is folded into the resolve: the HDR target is never written;
//   * the resolve hands a tile's codes through LDS, so that a wave stores one 256 B row segment of the row-major image;
//   * the tone curve is a template parameter: only the LPM instantiation loads the control block.
// Every level stored is rounded to half where the reference stores to its RGBA16F target.  Wave64, no scratch.
#include <algorithm>
#include <cmath>

#include "brmi_display_math.h"
#include "brmi_internal.h"

namespace brmi {

namespace dm = display;

struct Level { uint2* texels; uint32_t W, H, tilesX; };      // an RGBA16F level in the tiled layout
BRMI_DEV dm::rgb load_rgb(const uint2* t, uint32_t i) {
    const uint2 v = t[i];
    return dm::rgb{dm::half_value(v.x & 0xFFFFu), dm::half_value(v.x >> 16), dm::half_value(v.y & 0xFFFFu)};
}
BRMI_DEV uint2 pack_rgba(dm::rgb c, uint32_t alphaBits) { return make_uint2(dm::half_bits(c.r) | (dm::half_bits(c.g) << 16), dm::half_bits(c.b) | (alphaBits << 16)); }
BRMI_DEV dm::rgb sample_bilinear(const Level& l, float u, float v) {
    const dm::Bilinear b = dm::bilinear_of(u, v, l.W, l.H);
    const dm::rgb t00 = load_rgb(l.texels, tiled_index(b.x0, b.y0, l.tilesX)), t10 = load_rgb(l.texels, tiled_index(b.x1, b.y0, l.tilesX));
    const dm::rgb t01 = load_rgb(l.texels, tiled_index(b.x0, b.y1, l.tilesX)), t11 = load_rgb(l.texels, tiled_index(b.x1, b.y1, l.tilesX));
    return dm::rgb{dm::bilinear_mix(t00.r, t10.r, t01.r, t11.r, b.fx, b.fy), dm::bilinear_mix(t00.g, t10.g, t01.g, t11.g, b.fx, b.fy), dm::bilinear_mix(t00.b, t10.b, t01.b, t11.b, b.fx, b.fy)};
}
// sample_for_upsample: the 9-tap tent around (u, v) with the radius (x, y)
BRMI_DEV dm::rgb sample_tent(const Level& src, float u, float v, float x, float y) {
    float r[9], g[9], b[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        float ox, oy;
        dm::bloom_tent_offset(k, ox, oy);
        const dm::rgb t = sample_bilinear(src, u + ox * x, v + oy * y);
        r[k] = t.r; g[k] = t.g; b[k] = t.b;
    }
    return dm::rgb{dm::bloom_tent_combine(r), dm::bloom_tent_combine(g), dm::bloom_tent_combine(b)};
}

// ---- LuminanceHistogramPass: a wave per tile, grid-stride; 256 bins per workgroup in LDS ----------------------------------------------------------------------
struct HistogramArgs { const uint2* hdr; uint32_t* histogram; uint32_t W, H, tilesX, tileCount; float minLog, invRange; };
__global__ void __launch_bounds__(256) k_lum_histogram(HistogramArgs a) {
    __shared__ uint32_t bins[256];
    bins[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wavesPerGrid = gridDim.x * 4u;
    for (uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6); tile < a.tileCount; tile += wavesPerGrid) {
        const uint32_t px = (tile % a.tilesX) * 8u + (lane >> 3), py = (tile / a.tilesX) * 8u + (lane & 7u);
        const bool inside = px < a.W && py < a.H;
        uint32_t bin = 0u;
        if (inside) { const dm::rgb c = load_rgb(a.hdr, tile * 64u + lane); bin = dm::luminance_bin(c.r, c.g, c.b, a.minLog, a.invRange); }
        const uint64_t active = __ballot(inside);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
        if (__ballot(inside && bin == first) == active && inside) {      // the tile's pixels share a bin: one add
            if (lane == (uint32_t)__ffsll((unsigned long long)active) - 1u) atomicAdd(&bins[bin], (uint32_t)__popcll(active));
        } else if (inside) atomicAdd(&bins[bin], 1u);
    }
    __syncthreads();
    const uint32_t n = bins[threadIdx.x];
    if (n != 0u) atomicAdd(&a.histogram[threadIdx.x], n);
}

// ---- LuminanceHistogramAveragePass: one workgroup; leaves the histogram zero; thread 0 adapts and writes the LPM control block --------------------------------
struct AverageArgs { uint32_t* histogram; float* adapted; uint32_t* control; float numPixels, minLog, range, timeCoefficient; };
__global__ void __launch_bounds__(256) k_lum_average(AverageArgs a) {
    __shared__ uint32_t sums[256];
    const uint32_t i = threadIdx.x;
    const uint32_t countForThisBin = a.histogram[i];
    sums[i] = countForThisBin * i;
    __syncthreads();
    a.histogram[i] = 0u;
    for (uint32_t cutoff = 128u; cutoff > 0u; cutoff >>= 1) {
        if (i < cutoff) sums[i] += sums[i + cutoff];
        __syncthreads();
    }
    if (i == 0u) {
        const float average = dm::average_luminance(sums[0], countForThisBin, a.numPixels, a.minLog, a.range);
        const float adapted = dm::adapt_luminance(*a.adapted, average, a.timeCoefficient);
        *a.adapted = adapted;
        dm::lpm_setup(adapted, a.control);
    }
}
// autoExposure 0: the control block of a given adapted luminance (the adapted-luminance word is not touched)
__global__ void __launch_bounds__(64) k_lpm_setup_fixed(uint32_t* control, float adapted) {
    if (threadIdx.x == 0u) dm::lpm_setup(adapted, control);
}

// ---- BloomSamplePass, downsample: a wave per 8x8 destination tile --------------------------------------------------------------------------------------------------
struct BloomArgs { Level src, dst; float x, y; };      // down: the source's texel size; up: the tent's radius
__global__ void __launch_bounds__(256) k_bloom_down(BloomArgs a) {
    const uint32_t dstTilesY = (a.dst.H + 7u) >> 3;
    const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (tile >= a.dst.tilesX * dstTilesY) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t px = (tile % a.dst.tilesX) * 8u + (lane >> 3), py = (tile / a.dst.tilesX) * 8u + (lane & 7u);
    if (px >= a.dst.W || py >= a.dst.H) return;
    const float u = ((float)px + 0.5f) / (float)a.dst.W, v = ((float)py + 0.5f) / (float)a.dst.H;
    float r[13], g[13], b[13];
#pragma unroll
    for (int k = 0; k < 13; k++) {
        float ox, oy;
        dm::bloom_down_offset(k, ox, oy);
        const dm::rgb t = sample_bilinear(a.src, u + ox * a.x, v + oy * a.y);
        r[k] = t.r; g[k] = t.g; b[k] = t.b;
    }
    dm::rgb d{dm::bloom_down_combine(r), dm::bloom_down_combine(g), dm::bloom_down_combine(b)};
    dm::bloom_down_tail(d);
    a.dst.texels[tile * 64u + lane] = pack_rgba(d, 0x3C00u);
}
// ---- BloomSamplePass, upsample: dst = half(dst + tent(src)), alpha 1 (One / Zero) ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bloom_up(BloomArgs a) {
    const uint32_t dstTilesY = (a.dst.H + 7u) >> 3;
    const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (tile >= a.dst.tilesX * dstTilesY) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t px = (tile % a.dst.tilesX) * 8u + (lane >> 3), py = (tile / a.dst.tilesX) * 8u + (lane & 7u);
    if (px >= a.dst.W || py >= a.dst.H) return;
    const float u = ((float)px + 0.5f) / (float)a.dst.W, v = ((float)py + 0.5f) / (float)a.dst.H;
    const dm::rgb tent = sample_tent(a.src, u, v, a.x, a.y);
    const uint32_t i = tile * 64u + lane;
    const dm::rgb old = load_rgb(a.dst.texels, i);
    a.dst.texels[i] = pack_rgba(dm::rgb{dm::bloom_add(old.r, tent.r), dm::bloom_add(old.g, tent.g), dm::bloom_add(old.b, tent.b)}, 0x3C00u);
}

// ---- BloomBlendPass + TonemappingPass: eight tiles of one tile row per workgroup, a wave per tile; the codes go through LDS and wave w stores row w ------------
struct ResolveArgs { const uint2* hdr; Level bloom1; uint2* blendedHdr; const uint32_t* control; uint32_t* ldr; uint32_t W, H, tilesX; float x, y; };
template <uint32_t CURVE, bool BLOOM>
__global__ void __launch_bounds__(512) k_display_resolve(ResolveArgs a) {
    __shared__ uint32_t codes[8][72];      // (72: the 64 lanes of a tile's transposed write fall into 64 banks)
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint32_t tx = blockIdx.x * 8u + wave, ty = blockIdx.y;
    dm::LpmParams lpm{};
    if (CURVE == dm::AMD_LPM) {      // written by an earlier launch: through the constant address space, 25 scalar words
        uint32_t w[25];
#pragma unroll
        for (int k = 0; k < 25; k++) w[k] = kconst(a.control)[k];
        lpm = dm::lpm_unpack(w);
    }
    if (tx < a.tilesX) {
        const uint32_t lx = lane >> 3, ly = lane & 7u, px = tx * 8u + lx, py = ty * 8u + ly;
        if (px < a.W && py < a.H) {
            const uint32_t i = (ty * a.tilesX + tx) * 64u + lane;
            const uint2 raw = a.hdr[i];
            dm::rgb c{dm::half_value(raw.x & 0xFFFFu), dm::half_value(raw.x >> 16), dm::half_value(raw.y & 0xFFFFu)};
            if (BLOOM) {
                const float u = ((float)px + 0.5f) / (float)a.W, v = ((float)py + 0.5f) / (float)a.H;
                const dm::rgb bloom = sample_tent(a.bloom1, u, v, a.x, a.y);
                c = dm::rgb{dm::bloom_blend(c.r, bloom.r), dm::bloom_blend(c.g, bloom.g), dm::bloom_blend(c.b, bloom.b)};
                if (a.blendedHdr) a.blendedHdr[i] = pack_rgba(c, raw.y >> 16);      // (.rgb is written: alpha stays)
            }
            codes[ly][wave * 8u + lx] = dm::ldr_pixel(dm::tone_map<CURVE>(c, lpm));
        }
    }
    __syncthreads();
    const uint32_t ox = blockIdx.x * 64u + lane, oy = ty * 8u + wave;
    if (ox < a.W && oy < a.H) a.ldr[(size_t)oy * a.W + ox] = codes[wave][lane];
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------------------------
void display_layout(uint32_t width, uint32_t height, brmi_display_layout* l) {
    *l = brmi_display_layout{};
    l->histogramOffset = 0u; l->adaptedLuminanceOffset = 1024u; l->controlBlockOffset = 1152u;      // 1024 + 128; the block ends at 1536
    uint64_t off = 1536u;
    if (dm::bloom_possible(width, height)) {
        l->bloomLevels = dm::bloom_level_count(width, height);
        for (uint32_t k = 0; k < l->bloomLevels; k++) {
            brmi_display_plane& pl = l->bloom[k];
            pl.width = dm::bloom_level_size(width, k + 1u); pl.height = dm::bloom_level_size(height, k + 1u);
            pl.offset = off; pl.bytes = (uint64_t)((pl.width + 7u) / 8u) * ((pl.height + 7u) / 8u) * 64u * 8u;
            off = (off + pl.bytes + 255u) & ~255ull;
        }
    }
    l->scratchBytes = off;
    l->ldrBytes = (uint64_t)width * height * 4u;
    l->blendedHdrBytes = (uint64_t)((width + 7u) / 8u) * ((height + 7u) / 8u) * 64u * 8u;
}
static Level level_of(const brmi_pass* p, uint32_t level) {      // 0: the pass's HDR target (the resolved image of a bound temporal stage); only read
    if (level == 0u) return Level{static_cast<uint2*>(const_cast<void*>(display_input_of(p))), p->cfg.width, p->cfg.height, p->tilesX};
    const brmi_display_plane& pl = p->display.layout.bloom[level - 1u];
    return Level{reinterpret_cast<uint2*>(static_cast<uint8_t*>(p->display.b.scratch) + pl.offset), pl.width, pl.height, (pl.width + 7u) / 8u};
}
template <typename T> static T* scratch_at(const brmi_pass* p, uint64_t off) { return reinterpret_cast<T*>(static_cast<uint8_t*>(p->display.b.scratch) + off); }

int launch_display_exposure(brmi_pass* p, hipStream_t s, bool histogramOnly) {
    const brmi_display_settings& st = p->display.b.settings;
    const brmi_display_layout& l = p->display.layout;
    uint32_t* control = scratch_at<uint32_t>(p, l.controlBlockOffset);
    if (!st.autoExposure) {
        hipLaunchKernelGGL(k_lpm_setup_fixed, dim3(1), dim3(64), 0, s, control, st.fixedAdaptedLuminance);
        BRMI_LAUNCH_CHECK(p, "k_lpm_setup_fixed");
        return BRMI_OK;
    }
    HistogramArgs h{};
    h.hdr = static_cast<const uint2*>(display_input_of(p)); h.histogram = scratch_at<uint32_t>(p, l.histogramOffset);
    h.W = p->cfg.width; h.H = p->cfg.height; h.tilesX = p->tilesX; h.tileCount = p->tilesX * p->tilesY;
    h.minLog = st.minLogLuminance; h.invRange = 1.0f / st.logLuminanceRange;
    const uint32_t groups = std::min((h.tileCount + 3u) / 4u, 1024u);      // every wave walks tiles: at 4K a workgroup adds its bins once for 126 tiles
    hipLaunchKernelGGL(k_lum_histogram, dim3(groups), dim3(256), 0, s, h);
    BRMI_LAUNCH_CHECK(p, "k_lum_histogram");
    if (histogramOnly) return BRMI_OK;
    AverageArgs a{h.histogram, scratch_at<float>(p, l.adaptedLuminanceOffset), control, (float)(p->cfg.width * p->cfg.height), st.minLogLuminance, st.logLuminanceRange, st.timeCoefficient};
    hipLaunchKernelGGL(k_lum_average, dim3(1), dim3(256), 0, s, a);
    BRMI_LAUNCH_CHECK(p, "k_lum_average");
    return BRMI_OK;
}
// One BloomSamplePass{mipIndex, isUpsample}: down, level mipIndex -> mipIndex + 1 with the taps one source texel apart; up, level mipIndex + 1 -> mipIndex with the
// radius's aspect the destination's.
int launch_display_bloom_pass(brmi_pass* p, uint32_t mipIndex, bool isUpsample, hipStream_t s) {
    auto grid_of = [](const Level& d) { return dim3((d.tilesX * ((d.H + 7u) / 8u) + 3u) / 4u); };
    if (!isUpsample) {
        BloomArgs a{level_of(p, mipIndex), level_of(p, mipIndex + 1u), 0.0f, 0.0f};
        a.x = 1.0f / (float)a.src.W; a.y = 1.0f / (float)a.src.H;
        hipLaunchKernelGGL(k_bloom_down, grid_of(a.dst), dim3(256), 0, s, a);
        BRMI_LAUNCH_CHECK(p, "k_bloom_down");
    } else {
        BloomArgs a{level_of(p, mipIndex + 1u), level_of(p, mipIndex), 0.0f, 0.0f};
        a.x = dm::kBloomRadius; a.y = dm::kBloomRadius * ((float)a.dst.W / (float)a.dst.H);
        hipLaunchKernelGGL(k_bloom_up, grid_of(a.dst), dim3(256), 0, s, a);
        BRMI_LAUNCH_CHECK(p, "k_bloom_up");
    }
    return BRMI_OK;
}
int launch_display_bloom(brmi_pass* p, hipStream_t s) {      // BuildBloomPipeline without its last pass, which brmi_display_resolve applies
    if (!p->display.b.settings.bloom) return BRMI_OK;
    const uint32_t levels = p->display.layout.bloomLevels;
    for (uint32_t i = 0; i < levels; i++) if (int rc = launch_display_bloom_pass(p, i, false, s)) return rc;
    for (uint32_t i = levels - 1u; i > 0u; i--) if (int rc = launch_display_bloom_pass(p, i, true, s)) return rc;
    return BRMI_OK;
}
template <bool BLOOM> static void launch_resolve_of(uint32_t curve, dim3 grid, hipStream_t s, const ResolveArgs& a) {
    switch (curve) {
        case dm::REINHARD_JODIE: hipLaunchKernelGGL((k_display_resolve<dm::REINHARD_JODIE, BLOOM>), grid, dim3(512), 0, s, a); break;
        case dm::KHRONOS_PBR_NEUTRAL: hipLaunchKernelGGL((k_display_resolve<dm::KHRONOS_PBR_NEUTRAL, BLOOM>), grid, dim3(512), 0, s, a); break;
        case dm::ACES_HILL: hipLaunchKernelGGL((k_display_resolve<dm::ACES_HILL, BLOOM>), grid, dim3(512), 0, s, a); break;
        case dm::AMD_LPM: hipLaunchKernelGGL((k_display_resolve<dm::AMD_LPM, BLOOM>), grid, dim3(512), 0, s, a); break;
        default: hipLaunchKernelGGL((k_display_resolve<dm::NONE, BLOOM>), grid, dim3(512), 0, s, a); break;
    }
}
int launch_display_resolve(brmi_pass* p, hipStream_t s) {
    const brmi_display_settings& st = p->display.b.settings;
    ResolveArgs a{};
    a.hdr = static_cast<const uint2*>(display_input_of(p));
    a.control = scratch_at<uint32_t>(p, p->display.layout.controlBlockOffset);
    a.ldr = static_cast<uint32_t*>(p->display.b.ldr);
    a.W = p->cfg.width; a.H = p->cfg.height; a.tilesX = p->tilesX;
    const dim3 grid((p->tilesX + 7u) / 8u, p->tilesY);
    if (st.bloom) {
        a.bloom1 = level_of(p, 1u); a.blendedHdr = static_cast<uint2*>(p->display.b.blendedHdr);
        a.x = dm::kBloomRadius; a.y = dm::kBloomRadius * ((float)a.W / (float)a.H);
        launch_resolve_of<true>(st.tonemapType, grid, s, a);
    } else launch_resolve_of<false>(st.tonemapType, grid, s, a);
    BRMI_LAUNCH_CHECK(p, "k_display_resolve");
    return BRMI_OK;
}

}  // namespace brmi
