// brmi_gtao.hip -- XeGTAO ambient occlusion for gfx950: depth prefilter, main pass, denoise.
//
// Restates BR/shaders/GTAO.hlsl and BR/shaders/Intel/XeGTAO.hlsli (XeGTAO_PrefilterDepths16x16 :580-715, XeGTAO_MainPass :242-577, XeGTAO_Denoise :717-864) and
// the host's GTAOUpdateConstants (BR/include/ThirdParty/XeGTAO.h:165-202) as the reference's BuildGTAOPipeline runs them: linear view depth as the source,
// XE_GTAO_USE_DEFAULT_CONSTANTS (radius multiplier 1.457, falloff range 0.615, distribution power 2, no thin-occluder term), FP32 depths, no bent normals.
// MI355X-first differences:
//   * every GatherRed and point SampleLevel is integer texel loads with clamped coordinates (no uv is formed for a gather; the source-depth uv scale drops out);
//   * every plane is in the surfaces' tiled 8x8 layout, so one wave of the main pass is one tile: the G-buffer reads and both byte stores are contiguous per wave;
//   * the frame's constants are kernel arguments (wave-uniform: they live in SGPRs), made on the host per launch from the last brmi_update;
//   * the denoiser reads the nine codes around each of a thread's two pixels directly: the shader's seven gathers are exactly those texels.
// Arithmetic: IEEE fp32 without contraction, operations in the shader's order, `round` = round-half-to-even; sin, cos, log2 and pow are the device library's.
// The prefilter, the edges and the denoiser are exact (the tests hold them bit for bit); the main pass's working term is held to a float64 restatement.
#include <algorithm>
#include <cmath>

#include "brmi_internal.h"

namespace brmi {

constexpr float kRadiusMultiplier = 1.457f, kFalloffRange = 0.615f, kFinalValuePower = 2.2f, kDepthMipSamplingOffset = 3.30f;
constexpr float kPi = 3.1415926535897932384626433832795f, kPiHalf = 1.5707963267948966192313216916398f;

struct GtaoArgs {
    const float* srcDepth; const float4* normals;
    float* d0; float* d1; float* d2; float* d3; float* d4;      // the five depth levels
    uint8_t* edges; uint8_t* term;                              // the main pass's outputs
    uint32_t W, H, tilesX, tilesY;
    float psx, psy, mulx, muly, addx, addy, mulPixX;            // ViewportPixelSize, NDCToViewMul, NDCToViewAdd, NDCToViewMul_x_PixelSize.x
    float effectRadius, falloffMul, falloffAdd;                 // the main pass's (radius * 1.457)
    float mipFalloffMul, mipFalloffAdd;                         // the depth filter's (0.75 * radius * 1.457)
    float view[3][3];                                           // (float3x3)mainCamera.view
    uint32_t noiseIndex, maxDepthLod;
};
struct GtaoDenoiseArgs { const uint8_t* term; const uint8_t* edges; uint8_t* out; uint32_t W, H, tilesX, tilesY; float blurAmount; };

BRMI_DEV uint32_t mip_size(uint32_t size, uint32_t level) { return max((size + (1u << level) - 1u) >> level, 1u); }      // XeGTAO_GetMipViewportSize
BRMI_DEV int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// XeGTAO_DepthMIPFilter.  A quad with an empty texel: the formula's own limit is taken explicitly -- the empty ones weigh 1, the others 0, so the average is
// "empty" -- because as written two empties sum to +inf.
BRMI_DEV float gtao_mip_filter(float d0, float d1, float d2, float d3, float mul, float add) {
    const float maxDepth = max2(max2(d0, d1), max2(d2, d3));
    if (as_u32(maxDepth) == BRMI_DEPTH_EMPTY_BITS) return maxDepth;
    const float w0 = sat((maxDepth - d0) * mul + add), w1 = sat((maxDepth - d1) * mul + add), w2 = sat((maxDepth - d2) * mul + add), w3 = sat((maxDepth - d3) * mul + add);
    const float weightSum = ((w0 + w1) + w2) + w3;
    return (((w0 * d0 + w1 * d1) + w2 * d2) + w3 * d3) / weightSum;
}
BRMI_DEV float gtao_clamp_depth(float d) { return min2(max2(d, 0.0f), 3.402823466e+38f); }      // XeGTAO_ClampDepth, the FP32 range (NaN and negatives: 0)

// One 16x16 block per workgroup of one wave; thread (tx, ty) owns the 2x2 pixels at (2 bx, 2 by).  Levels 2-4 go through LDS as in the shader.
__global__ void __launch_bounds__(64) k_gtao_prefilter(GtaoArgs a) {
    __shared__ float scratchDepths[8][8];
    const uint32_t tx = threadIdx.x >> 3, ty = threadIdx.x & 7u;
    const uint32_t bx = blockIdx.x * 8u + tx, by = blockIdx.y * 8u + ty;
    const uint32_t px = bx * 2u, py = by * 2u;
    // GatherRed at the clamped pixel with offset (1, 1): texels (cx .. cx + 1, cy .. cy + 1), clamped
    const uint32_t cx = min(px, a.W - 1u), cy = min(py, a.H - 1u), cx1 = min(cx + 1u, a.W - 1u), cy1 = min(cy + 1u, a.H - 1u);
    const float depth0 = gtao_clamp_depth(a.srcDepth[tiled_index(cx, cy, a.tilesX)]), depth1 = gtao_clamp_depth(a.srcDepth[tiled_index(cx1, cy, a.tilesX)]);
    const float depth2 = gtao_clamp_depth(a.srcDepth[tiled_index(cx, cy1, a.tilesX)]), depth3 = gtao_clamp_depth(a.srcDepth[tiled_index(cx1, cy1, a.tilesX)]);
    if (px < a.W && py < a.H) a.d0[tiled_index(px, py, a.tilesX)] = depth0;
    if (px + 1u < a.W && py < a.H) a.d0[tiled_index(px + 1u, py, a.tilesX)] = depth1;
    if (px < a.W && py + 1u < a.H) a.d0[tiled_index(px, py + 1u, a.tilesX)] = depth2;
    if (px + 1u < a.W && py + 1u < a.H) a.d0[tiled_index(px + 1u, py + 1u, a.tilesX)] = depth3;
    const float dm1 = gtao_mip_filter(depth0, depth1, depth2, depth3, a.mipFalloffMul, a.mipFalloffAdd);
    { const uint32_t w = mip_size(a.W, 1u), h = mip_size(a.H, 1u); if (bx < w && by < h) a.d1[tiled_index(bx, by, (w + 7u) >> 3)] = dm1; }
    scratchDepths[tx][ty] = dm1;
    __syncthreads();
    if ((tx & 1u) == 0u && (ty & 1u) == 0u) {
        const float dm2 = gtao_mip_filter(scratchDepths[tx][ty], scratchDepths[tx + 1u][ty], scratchDepths[tx][ty + 1u], scratchDepths[tx + 1u][ty + 1u], a.mipFalloffMul, a.mipFalloffAdd);
        const uint32_t w = mip_size(a.W, 2u), h = mip_size(a.H, 2u), x = bx >> 1, y = by >> 1;
        if (x < w && y < h) a.d2[tiled_index(x, y, (w + 7u) >> 3)] = dm2;
        scratchDepths[tx][ty] = dm2;
    }
    __syncthreads();
    if ((tx & 3u) == 0u && (ty & 3u) == 0u) {
        const float dm3 = gtao_mip_filter(scratchDepths[tx][ty], scratchDepths[tx + 2u][ty], scratchDepths[tx][ty + 2u], scratchDepths[tx + 2u][ty + 2u], a.mipFalloffMul, a.mipFalloffAdd);
        const uint32_t w = mip_size(a.W, 3u), h = mip_size(a.H, 3u), x = bx >> 2, y = by >> 2;
        if (x < w && y < h) a.d3[tiled_index(x, y, (w + 7u) >> 3)] = dm3;
        scratchDepths[tx][ty] = dm3;
    }
    __syncthreads();
    if (tx == 0u && ty == 0u) {
        const float dm4 = gtao_mip_filter(scratchDepths[0][0], scratchDepths[4][0], scratchDepths[0][4], scratchDepths[4][4], a.mipFalloffMul, a.mipFalloffAdd);
        const uint32_t w = mip_size(a.W, 4u), h = mip_size(a.H, 4u), x = bx >> 3, y = by >> 3;
        if (x < w && y < h) a.d4[tiled_index(x, y, (w + 7u) >> 3)] = dm4;
    }
}

// XeGTAO_FastSqrt / XeGTAO_FastACos: part of the definition, the bit trick on the fp32 pattern included (asint(x) >> 1 is an arithmetic shift)
BRMI_DEV float gtao_fast_sqrt(float x) { return as_f32(0x1fbd1df5u + (uint32_t)((int32_t)as_u32(x) >> 1)); }
BRMI_DEV float gtao_fast_acos(float inX) {
    const float x = fabsf(inX);
    float res = -0.156583f * x + 1.570796f;
    res = res * gtao_fast_sqrt(1.0f - x);
    return inX >= 0.0f ? res : 3.141593f - res;
}
BRMI_DEV uint32_t gtao_hilbert_index(uint32_t posX, uint32_t posY) {      // HilbertIndex (XeGTAO.h:121-143), level 6; only the low six bits of a coordinate take part
    posX &= 63u; posY &= 63u;
    uint32_t index = 0u;
#pragma unroll
    for (uint32_t curLevel = 32u; curLevel > 0u; curLevel >>= 1) {
        const uint32_t regionX = (posX & curLevel) > 0u ? 1u : 0u, regionY = (posY & curLevel) > 0u ? 1u : 0u;
        index += curLevel * curLevel * ((3u * regionX) ^ regionY);
        if (regionY == 0u) {
            if (regionX == 1u) { posX = 63u - posX; posY = 63u - posY; }
            const uint32_t temp = posX; posX = posY; posY = temp;
        }
    }
    return index;
}
BRMI_DEV float gtao_frac(float x) { return x - floorf(x); }

// XeGTAO_CalculateEdges + XeGTAO_PackEdges, then the R8_UNORM store's code (round to nearest)
BRMI_DEV uint32_t gtao_edges_code(float centerZ, float leftZ, float rightZ, float topZ, float bottomZ) {
    float e[4] = {leftZ - centerZ, rightZ - centerZ, topZ - centerZ, bottomZ - centerZ};
    const float slopeLR = (e[1] - e[0]) * 0.5f, slopeTB = (e[3] - e[2]) * 0.5f;
    const float adj[4] = {e[0] + slopeLR, e[1] + -slopeLR, e[2] + slopeTB, e[3] + -slopeTB};
    const float den = centerZ * 0.011f;
    float packed[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float m = min2(fabsf(e[k]), fabsf(adj[k]));
        packed[k] = rintf(sat(sat(1.25f - m / den)) * 2.9f);
    }
    const float v = ((packed[0] * (float)(64.0 / 255.0) + packed[1] * (float)(16.0 / 255.0)) + packed[2] * (float)(4.0 / 255.0)) + packed[3] * (float)(1.0 / 255.0);
    return (uint32_t)(sat(v) * 255.0f + 0.5f);
}

// One wave per 8x8 tile (four tiles per workgroup); the lane is the pixel at tile-local (lane >> 3, lane & 7), which is also its place in the tile's 64 bytes.
template <int SLICES, int STEPS>
__global__ void __launch_bounds__(256) k_gtao_main(GtaoArgs a) {
    const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (tile >= a.tilesX * a.tilesY) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int px = (int)((tile % a.tilesX) * 8u + (lane >> 3)), py = (int)((tile / a.tilesX) * 8u + (lane & 7u));
    if (px >= (int)a.W || py >= (int)a.H) return;
    const uint32_t i = tile * 64u + lane;
    const int maxX = (int)a.W - 1, maxY = (int)a.H - 1;
    auto depth0_at = [&](int x, int y) -> float { return a.d0[tiled_index((uint32_t)clampi(x, 0, maxX), (uint32_t)clampi(y, 0, maxY), a.tilesX)]; };
    // the two gathers: centre, left, top from the one at the pixel's corner, right and bottom from the one at offset (1, 1)
    float viewspaceZ = depth0_at(px, py);
    const float pixLZ = depth0_at(px - 1, py), pixTZ = depth0_at(px, py - 1), pixRZ = depth0_at(px + 1, py), pixBZ = depth0_at(px, py + 1);
    a.edges[i] = (uint8_t)gtao_edges_code(viewspaceZ, pixLZ, pixRZ, pixTZ, pixBZ);
    // an empty centre pixel: visibility 1 through XeGTAO_OutputWorkingTerm (the text's own value there depends on how NaN travels)
    if (as_u32(viewspaceZ) == BRMI_DEPTH_EMPTY_BITS) { a.term[i] = (uint8_t)170u; return; }

    // LoadNormal: the world normal through (float3x3)view, normalised, z flipped
    const float4 nw = a.normals[i];
    f3 viewspaceNormal = normalize3_q(f3{(nw.x * a.view[0][0] + nw.y * a.view[1][0]) + nw.z * a.view[2][0], (nw.x * a.view[0][1] + nw.y * a.view[1][1]) + nw.z * a.view[2][1],
                                         (nw.x * a.view[0][2] + nw.y * a.view[1][2]) + nw.z * a.view[2][2]});
    viewspaceNormal.z = -viewspaceNormal.z;
    // SpatioTemporalNoise: Hilbert index driving R2
    const uint32_t noiseIdx = gtao_hilbert_index((uint32_t)px, (uint32_t)py) + 288u * a.noiseIndex;
    const float noiseSlice = gtao_frac(0.5f + (float)noiseIdx * 0.75487766624669276005f), noiseSample = gtao_frac(0.5f + (float)noiseIdx * 0.5698402909980532659114f);

    const float nspx = ((float)px + 0.5f) * a.psx, nspy = ((float)py + 0.5f) * a.psy;      // normalizedScreenPos
    viewspaceZ = viewspaceZ * 0.99999f;
    const f3 pixCenterPos{(a.mulx * nspx + a.addx) * viewspaceZ, (a.muly * nspy + a.addy) * viewspaceZ, viewspaceZ};
    const f3 viewVec = normalize3_q(-pixCenterPos);
    const float screenspaceRadius = a.effectRadius / (viewspaceZ * a.mulPixX);
    float visibility = sat((10.0f - screenspaceRadius) / 100.0f) * 0.5f;
    const float minS = 1.3f / screenspaceRadius;

    // a tap on one side of the slice: the horizon it leaves.  An empty texel leaves the horizon as it is (weight 0 in the formula's own limit).
    auto tap = [&](float rx, float ry, float sign, uint32_t level, float lowHorizonCos, float horizonCos) -> float {
        const float spx = nspx + sign * (rx * a.psx), spy = nspy + sign * (ry * a.psy);      // sampleScreenPos
        float SZ;
        if (level == 0u) SZ = depth0_at(px + (int)(sign * rx), py + (int)(sign * ry));
        else {
            const uint32_t lw = mip_size(a.W, level), lh = mip_size(a.H, level);
            const float* lp = level == 1u ? a.d1 : level == 2u ? a.d2 : level == 3u ? a.d3 : a.d4;
            const int tx = clampi((int)floorf(clampf(spx * (float)lw, -1.0f, 65536.0f)), 0, (int)lw - 1), ty = clampi((int)floorf(clampf(spy * (float)lh, -1.0f, 65536.0f)), 0, (int)lh - 1);
            SZ = lp[tiled_index((uint32_t)tx, (uint32_t)ty, (lw + 7u) >> 3)];
        }
        if (as_u32(SZ) == BRMI_DEPTH_EMPTY_BITS) return horizonCos;
        const f3 samplePos{(a.mulx * spx + a.addx) * SZ, (a.muly * spy + a.addy) * SZ, SZ};
        const f3 sampleDelta = samplePos - pixCenterPos;
        const float sampleDist = sqrtf(dot3(sampleDelta, sampleDelta));
        const f3 sampleHorizonVec = sampleDelta / sampleDist;
        const float weight = sat(sampleDist * a.falloffMul + a.falloffAdd);
        float shc = dot3(sampleHorizonVec, viewVec);
        shc = lowHorizonCos + weight * (shc - lowHorizonCos);      // lerp(low, shc, weight)
        return max2(horizonCos, shc);
    };

#pragma unroll 1
    for (int sl = 0; sl < SLICES; sl++) {
        const float slice = (float)sl;
        const float sliceK = (slice + noiseSlice) / (float)SLICES;
        const float phi = sliceK * kPi;
        const float cosPhi = cosf(phi), sinPhi = sinf(phi);
        const float omegaX = cosPhi * screenspaceRadius, omegaY = -sinPhi * screenspaceRadius;
        const f3 directionVec{cosPhi, sinPhi, 0.0f};
        const f3 orthoDirectionVec = directionVec - (cosPhi * viewVec.x + sinPhi * viewVec.y) * viewVec;
        const f3 axisVec = normalize3_q(cross3(orthoDirectionVec, viewVec));
        const f3 projectedNormalVec = viewspaceNormal - axisVec * dot3(viewspaceNormal, axisVec);
        const float sd = dot3(orthoDirectionVec, projectedNormalVec);
        const float signNorm = sd > 0.0f ? 1.0f : (sd < 0.0f ? -1.0f : 0.0f);
        float projectedNormalVecLength = sqrtf(dot3(projectedNormalVec, projectedNormalVec));
        const float cosNorm = sat(dot3(projectedNormalVec, viewVec) / projectedNormalVecLength);
        const float n = signNorm * gtao_fast_acos(cosNorm);
        const float lowHorizonCos0 = cosf(n + kPiHalf), lowHorizonCos1 = cosf(n - kPiHalf);
        float horizonCos0 = lowHorizonCos0, horizonCos1 = lowHorizonCos1;
#pragma unroll
        for (int st = 0; st < STEPS; st++) {
            const float stepBaseNoise = (float)(sl + st * STEPS) * 0.6180339887498948482f;
            const float stepNoise = gtao_frac(noiseSample + stepBaseNoise);
            float s = ((float)st + stepNoise) / (float)STEPS;
            s = s * s;      // pow(s, XE_GTAO_DEFAULT_SAMPLE_DISTRIBUTION_POWER = 2)
            s = s + minS;
            const float sox = s * omegaX, soy = s * omegaY;
            uint32_t level = 0u;
            if (a.maxDepthLod != 0u) {      // (wave-uniform.  The reference's sampler clamps the level to its maxLod; nearest level = floor(lod + 0.5))
                const float sampleOffsetLength = sqrtf(sox * sox + soy * soy);
                const float mipLevel = min2(clampf(log2f(sampleOffsetLength) - kDepthMipSamplingOffset, 0.0f, 5.0f), (float)a.maxDepthLod);
                level = (uint32_t)floorf(mipLevel + 0.5f);
            }
            // round() to the texel centre; the clamp keeps the integer texel offset of a huge screen radius representable (it lands on the frame's edge either way)
            const float rx = clampf(rintf(sox), -65536.0f, 65536.0f), ry = clampf(rintf(soy), -65536.0f, 65536.0f);
            horizonCos0 = tap(rx, ry, 1.0f, level, lowHorizonCos0, horizonCos0);
            horizonCos1 = tap(rx, ry, -1.0f, level, lowHorizonCos1, horizonCos1);
        }
        projectedNormalVecLength = projectedNormalVecLength + 0.05f * (1.0f - projectedNormalVecLength);      // lerp(len, 1, 0.05)
        const float h0 = -gtao_fast_acos(horizonCos1), h1 = gtao_fast_acos(horizonCos0);
        const float sinN = sinf(n);
        const float iarc0 = ((cosNorm + (2.0f * h0) * sinN) - cosf(2.0f * h0 - n)) / 4.0f;
        const float iarc1 = ((cosNorm + (2.0f * h1) * sinN) - cosf(2.0f * h1 - n)) / 4.0f;
        visibility = visibility + projectedNormalVecLength * (iarc0 + iarc1);
    }
    visibility = visibility / (float)SLICES;
    visibility = visibility > 0.0f ? powf(visibility, kFinalValuePower) : 0.0f;      // (pow of a non-positive base: NaN or 0 in the text, and max() below returns 0.03 for both)
    visibility = max2(0.03f, visibility);
    a.term[i] = (uint8_t)(uint32_t)(sat(visibility / 1.5f) * 255.0f + 0.5f);      // XeGTAO_OutputWorkingTerm
}

// XeGTAO_UnpackEdges of an R8_UNORM code
BRMI_DEV void gtao_unpack_edges(uint32_t code, float e[4]) {
    const uint32_t packedVal = (uint32_t)(((float)code / 255.0f) * 255.5f);
    e[0] = sat((float)((packedVal >> 6) & 3u) / 3.0f); e[1] = sat((float)((packedVal >> 4) & 3u) / 3.0f);
    e[2] = sat((float)((packedVal >> 2) & 3u) / 3.0f); e[3] = sat((float)(packedVal & 3u) / 3.0f);
}
// One pixel of XeGTAO_Denoise: the shader's gathers, side by side, are the 3x3 codes around the pixel with clamped coordinates.
template <bool FINAL>
BRMI_DEV uint32_t gtao_denoise_pixel(const GtaoDenoiseArgs& a, int x, int y) {
    const int maxX = (int)a.W - 1, maxY = (int)a.H - 1;
    auto at = [&](int xx, int yy) { return tiled_index((uint32_t)clampi(xx, 0, maxX), (uint32_t)clampi(yy, 0, maxY), a.tilesX); };
    auto vis = [&](int xx, int yy) { return (float)a.term[at(xx, yy)] / 255.0f; };
    float C[4], L[4], R[4], T[4], B[4];
    gtao_unpack_edges(a.edges[at(x, y)], C); gtao_unpack_edges(a.edges[at(x - 1, y)], L); gtao_unpack_edges(a.edges[at(x + 1, y)], R);
    gtao_unpack_edges(a.edges[at(x, y - 1)], T); gtao_unpack_edges(a.edges[at(x, y + 1)], B);
    C[0] = C[0] * L[1]; C[1] = C[1] * R[0]; C[2] = C[2] * T[3]; C[3] = C[3] * B[2];
    const float edginess = (sat(1.5f - (((C[0] + C[1]) + C[2]) + C[3])) / 1.5f) * 0.5f;      // leak_threshold 2.5, leak_strength 0.5
#pragma unroll
    for (int k = 0; k < 4; k++) C[k] = sat(C[k] + edginess);
    const float diagWeight = 0.425f;      // 0.85 * 0.5
    const float weightTL = diagWeight * (C[0] * L[2] + C[2] * T[0]), weightTR = diagWeight * (C[2] * T[1] + C[1] * R[2]);
    const float weightBL = diagWeight * (C[3] * B[0] + C[0] * L[3]), weightBR = diagWeight * (C[1] * R[3] + C[3] * B[1]);
    float sumWeight = a.blurAmount;
    float sum = vis(x, y) * sumWeight;
    auto add = [&](float v, float w) { sum = sum + w * v; sumWeight = sumWeight + w; };
    add(vis(x - 1, y), C[0]); add(vis(x + 1, y), C[1]); add(vis(x, y - 1), C[2]); add(vis(x, y + 1), C[3]);
    add(vis(x - 1, y - 1), weightTL); add(vis(x + 1, y - 1), weightTR); add(vis(x - 1, y + 1), weightBL); add(vis(x + 1, y + 1), weightBR);
    float ao = sum / sumWeight;
    if (FINAL) ao = ao * 1.5f;      // XE_GTAO_OCCLUSION_TERM_SCALE
    return min((uint32_t)(ao * 255.0f + 0.5f), 255u);      // (the R8_UINT store saturates)
}
// Each thread handles two horizontal pixels, as the shader does; a wave covers two neighbouring tiles (16 x 8 pixels), lane = (pair column, row).
template <bool FINAL>
__global__ void __launch_bounds__(256) k_gtao_denoise(GtaoDenoiseArgs a) {
    const uint32_t pairsX = (a.tilesX + 1u) >> 1;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (wave >= pairsX * a.tilesY) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int bx = (int)((wave % pairsX) * 16u + (lane >> 3) * 2u), y = (int)((wave / pairsX) * 8u + (lane & 7u));
    if (bx >= (int)a.W || y >= (int)a.H) return;
    a.out[tiled_index((uint32_t)bx, (uint32_t)y, a.tilesX)] = (uint8_t)gtao_denoise_pixel<FINAL>(a, bx, y);
    if (bx + 1 < (int)a.W) a.out[tiled_index((uint32_t)bx + 1u, (uint32_t)y, a.tilesX)] = (uint8_t)gtao_denoise_pixel<FINAL>(a, bx + 1, y);
}

// ---- host ----
void gtao_layout(uint32_t width, uint32_t height, brmi_gtao_layout* l) {
    *l = brmi_gtao_layout{};
    uint64_t off = 0;
    auto plane = [&](brmi_gtao_plane& pl, uint32_t w, uint32_t h, uint32_t bytesPerPixel) {
        pl.offset = off; pl.width = w; pl.height = h;
        off += (uint64_t)((w + 7u) / 8u) * ((h + 7u) / 8u) * 64u * bytesPerPixel;
        off = (off + 255u) & ~255ull;
    };
    for (uint32_t m = 0; m < 5u; m++) plane(l->depth[m], std::max((width + (1u << m) - 1u) >> m, 1u), std::max((height + (1u << m) - 1u) >> m, 1u), 4u);
    plane(l->edges, width, height, 1u); plane(l->term[0], width, height, 1u); plane(l->term[1], width, height, 1u);
    l->scratchBytes = off;
    l->outputBytes = (uint64_t)((width + 7u) / 8u) * ((height + 7u) / 8u) * 64u;
}

// GTAOUpdateConstants from the last brmi_update's main camera (fov, aspectRatio) and the frame size, in fp32 as the reference's host has them; tan through the
// double-precision function so that the value does not depend on a float math library.
static GtaoArgs gtao_args_of(const brmi_pass* p) {
    GtaoArgs a{};
    uint8_t* scratch = static_cast<uint8_t*>(p->gtao.b.scratch);
    const brmi_gtao_layout& l = p->gtao.layout;
    a.srcDepth = static_cast<const float*>(p->res[BRMI_RES_LINEAR_DEPTH]); a.normals = static_cast<const float4*>(p->res[BRMI_RES_GBUF_NORMALS]);
    a.d0 = reinterpret_cast<float*>(scratch + l.depth[0].offset); a.d1 = reinterpret_cast<float*>(scratch + l.depth[1].offset); a.d2 = reinterpret_cast<float*>(scratch + l.depth[2].offset);
    a.d3 = reinterpret_cast<float*>(scratch + l.depth[3].offset); a.d4 = reinterpret_cast<float*>(scratch + l.depth[4].offset);
    a.edges = scratch + l.edges.offset; a.term = scratch + l.term[0].offset;
    a.W = p->cfg.width; a.H = p->cfg.height; a.tilesX = p->tilesX; a.tilesY = p->tilesY;
    a.psx = 1.0f / (float)a.W; a.psy = 1.0f / (float)a.H;
    const float tanHalfFOVY = (float)std::tan((double)(p->camHost.fov * 0.5f)), tanHalfFOVX = tanHalfFOVY * p->camHost.aspectRatio;
    a.mulx = tanHalfFOVX * 2.0f; a.muly = tanHalfFOVY * -2.0f; a.addx = tanHalfFOVX * -1.0f; a.addy = tanHalfFOVY * 1.0f;
    a.mulPixX = a.mulx * a.psx;
    const float radius = p->gtao.b.settings.radius;
    {   // XeGTAO_MainPass :301-317
        const float effectRadius = radius * kRadiusMultiplier, falloffRange = kFalloffRange * effectRadius, falloffFrom = effectRadius * (1.0f - kFalloffRange);
        a.effectRadius = effectRadius; a.falloffMul = -1.0f / falloffRange; a.falloffAdd = falloffFrom / falloffRange + 1.0f;
    }
    {   // XeGTAO_DepthMIPFilter :584-595
        const float effectRadius = 0.75f * radius * kRadiusMultiplier, falloffRange = kFalloffRange * effectRadius, falloffFrom = effectRadius * (1.0f - kFalloffRange);
        a.mipFalloffMul = -1.0f / falloffRange; a.mipFalloffAdd = falloffFrom / falloffRange + 1.0f;
    }
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) a.view[r][c] = p->camHost.view[r][c];
    a.noiseIndex = p->frameIndexHost % 64u; a.maxDepthLod = p->gtao.b.settings.maxDepthLod;
    return a;
}

int launch_gtao_prefilter(brmi_pass* p, hipStream_t s) {
    const GtaoArgs a = gtao_args_of(p);
    hipLaunchKernelGGL(k_gtao_prefilter, dim3((a.W + 15u) / 16u, (a.H + 15u) / 16u), dim3(64), 0, s, a);
    BRMI_LAUNCH_CHECK(p, "k_gtao_prefilter");
    return BRMI_OK;
}
int launch_gtao_main(brmi_pass* p, hipStream_t s) {
    const GtaoArgs a = gtao_args_of(p);
    const dim3 grid((a.tilesX * a.tilesY + 3u) / 4u);
    switch (p->gtao.b.settings.qualityLevel) {
        case 0: hipLaunchKernelGGL((k_gtao_main<1, 2>), grid, dim3(256), 0, s, a); break;
        case 1: hipLaunchKernelGGL((k_gtao_main<2, 2>), grid, dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_gtao_main<3, 3>), grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((k_gtao_main<9, 3>), grid, dim3(256), 0, s, a); break;
    }
    BRMI_LAUNCH_CHECK(p, "k_gtao_main");
    return BRMI_OK;
}
int launch_gtao_denoise(brmi_pass* p, hipStream_t s) {
    uint8_t* scratch = static_cast<uint8_t*>(p->gtao.b.scratch);
    const brmi_gtao_layout& l = p->gtao.layout;
    uint8_t* term[2] = {scratch + l.term[0].offset, scratch + l.term[1].offset};
    const uint32_t passes = p->gtao.b.settings.denoisePasses;
    const float beta = passes == 0u ? 1e4f : 1.2f;      // DenoiseBlurBeta
    GtaoDenoiseArgs a{};
    a.edges = scratch + l.edges.offset; a.W = p->cfg.width; a.H = p->cfg.height; a.tilesX = p->tilesX; a.tilesY = p->tilesY;
    const dim3 grid((((a.tilesX + 1u) / 2u) * a.tilesY + 3u) / 4u);
    uint32_t src = 0u;
    for (uint32_t k = 1u; k < passes; k++) {      // the non-final passes ping-pong between the two working terms
        a.term = term[src]; a.out = term[src ^ 1u]; a.blurAmount = beta / 5.0f;
        hipLaunchKernelGGL(k_gtao_denoise<false>, grid, dim3(256), 0, s, a);
        BRMI_LAUNCH_CHECK(p, "k_gtao_denoise<false>");
        src ^= 1u;
    }
    a.term = term[src]; a.out = static_cast<uint8_t*>(p->gtao.b.aoTerm); a.blurAmount = beta;
    hipLaunchKernelGGL(k_gtao_denoise<true>, grid, dim3(256), 0, s, a);
    BRMI_LAUNCH_CHECK(p, "k_gtao_denoise<true>");
    return BRMI_OK;
}

}  // namespace brmi
