// brmi_envbuild.hip -- the environment build for gfx950: equirectangular image -> cube, cube -> irradiance SH integers, cube -> GGX-prefiltered RGBA8 chain.
//
// Reference: BR/shaders/envToCubemap.hlsl, BR/shaders/sphericalHarmonics.hlsl, BR/shaders/blurEnvironment.hlsl, the loop of
// BR/include/RenderPasses/EnvironmentFilterPass.h:99-127, BR/src/Scene/Environment.cpp:29-33.
// MI355X-first differences:
//   * one launch per stage: faces (and, in the prefilter, levels) ride in the grid; the reference dispatches per face and per (level, face);
//   * a workgroup is a 16 x 16 texel tile of one face, a wave an 8 x 8 quarter of it: the lookups of a wave land on neighbouring source texels;
//   * the SH projection adds its 27 integers across the wave with shuffles, across the workgroup through LDS, and issues 27 atomics per WORKGROUP where the
//     reference issues 27 per texel on one 128 B record (atomics on one line serialise: DESIGN.md 8 item 0(c)).  Integer sums: the result is the reference's
//     whatever the order;
//   * the prefilter's 16 half vectors in tangent space depend on the level alone (Hammersley point, roughness): sixteen lanes compute them once per workgroup
//     into LDS, and a texel's loop only rotates them into its frame.
// Arithmetic: IEEE fp32, no contraction; normalize(v) = v * (1 / sqrt(dot(v, v))), both correctly rounded (brmi_device.h, normalize3_q); sin, cos, atan2, asin
// are the device library's.  A value is kept from fusing into its fp16 conversion (v_fma_mix would round once where the shader rounds twice).
#include <algorithm>

#include "brmi_internal.h"
#include "brmi_texture.h"

namespace brmi {

constexpr float kPi = 3.14159265359f;      // the PI of the three shaders

BRMI_DEV float opaque(float x) { asm volatile("" : "+v"(x)); return x; }
// the texel of a 16 x 16 tile this thread owns: wave w is the 8 x 8 quarter (w & 1, w >> 1), a lane one texel of it, eight lanes along a row
BRMI_DEV void tile_texel(uint32_t tileX, uint32_t tileY, uint32_t& x, uint32_t& y) {
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    x = tileX * 16u + (w & 1u) * 8u + (lane & 7u); y = tileY * 16u + (w >> 1) * 8u + (lane >> 3);
}
// FaceUVToDir of envToCubemap.hlsl / blurEnvironment.hlsl (uv in [-1, 1], y already flipped)
BRMI_DEV f3 face_uv_to_dir(uint32_t face, float u, float v) {
    switch (face) {
        case 0: return normalize3_q(f3{1.0f, v, -u});
        case 1: return normalize3_q(f3{-1.0f, v, u});
        case 2: return normalize3_q(f3{u, 1.0f, -v});
        case 3: return normalize3_q(f3{u, -1.0f, v});
        case 4: return normalize3_q(f3{u, v, 1.0f});
        default: return normalize3_q(f3{-u, v, -1.0f});
    }
}
// level `level` of a destination face: false when the descriptor cannot take texel (x, y) of it in `format`
// (the descriptor through the scalar path, field by field: a local copy indexed by the level would live in scratch)
typedef const __attribute__((address_space(4))) brmi_texture_desc* KDesc;
BRMI_DEV bool dst_texel(KDesc d, uint32_t format, uint32_t level, uint32_t x, uint32_t y, uint8_t*& texels, size_t& index) {
    texels = const_cast<uint8_t*>(d->texels);
    const uint32_t width = d->width, height = d->height, mipCount = d->mipCount;
    if (texels == nullptr || d->format != format || mipCount == 0u || mipCount > BRMI_TEXTURE_MAX_MIPS || level >= mipCount) return false;
    const uint32_t w = width >> level ? width >> level : 1u, h = height >> level ? height >> level : 1u;
    if (width == 0u || height == 0u || x >= w || y >= h) return false;
    index = (size_t)d->mipOffset[level] + (size_t)y * w + x;
    return true;
}

// ================================================ envToCubemap ================================================
__global__ void __launch_bounds__(256) k_env_convert(const brmi_texture_desc* equirect, const brmi_texture_desc* cube, uint32_t size) {
    __shared__ float texelTables[256];
    stage_unorm_table(texelTables, threadIdx.x, 256u); __syncthreads();
    TexelTables tb; tb.t = texelTables;
    uint32_t x, y; tile_texel(blockIdx.x, blockIdx.y, x, y);
    const uint32_t face = blockIdx.z;
    if (x >= size || y >= size) return;
    const float u = ((float)x + 0.5f) / (float)size * 2.0f - 1.0f, v = -(((float)y + 0.5f) / (float)size * 2.0f - 1.0f);
    const f3 dir = normalize3_q(face_uv_to_dir(face, u, v));      // (DirToEquirect normalises again)
    const f2 eq{atan2f(dir.z, dir.x) / (2.0f * kPi) + 0.5f, 0.5f - asinf(dir.y) / kPi};
    const f4 c = sample_desc_level_any(tb, kconst(equirect), eq, 0.0f);
    uint8_t* texels; size_t index;
    if (!dst_texel(kconst(cube + face), BRMI_TEXTURE_FORMAT_RGBA16_FLOAT, 0u, x, y, texels, index)) return;
    const uint2 out = make_uint2(f32_to_f16_bits(opaque(c.x)) | (f32_to_f16_bits(opaque(c.y)) << 16), f32_to_f16_bits(opaque(c.z)) | (0x3C00u << 16));
    reinterpret_cast<uint2*>(texels)[index] = out;
}

// ================================================ sphericalHarmonics ================================================
__global__ void __launch_bounds__(64) k_env_sh_reset(brmi_environment_info* env, float scale) {
    if (threadIdx.x < 27u) env->sphericalHarmonics[threadIdx.x] = 0;
    if (threadIdx.x == 27u) env->sphericalHarmonicsScale = scale;
}
__global__ void __launch_bounds__(256) k_env_project_sh(const brmi_texture_desc* cubemaps, uint32_t cubemapCount, brmi_environment_info* env, uint32_t size) {
    __shared__ float texelTables[256];
    __shared__ uint32_t partial[4][27];
    stage_unorm_table(texelTables, threadIdx.x, 256u); __syncthreads();
    TexelTables tb; tb.t = texelTables;
    uint32_t x, y; tile_texel(blockIdx.x, blockIdx.y, x, y);
    const uint32_t face = blockIdx.z;
    const uint32_t cubemap = kconst(env)->cubeMapDescriptorIndex;
    uint32_t acc[27];
#pragma unroll
    for (int k = 0; k < 27; k++) acc[k] = 0u;
    if (x < size && y < size) {
        const float u = ((float)x + 0.5f) / (float)size * 2.0f - 1.0f, v = ((float)y + 0.5f) / (float)size * 2.0f - 1.0f;
        f3 dir;
        switch (face) {      // the file's own table (the Direct3D cube layout)
            case 0: dir = f3{1.0f, -v, -u}; break;
            case 1: dir = f3{-1.0f, -v, u}; break;
            case 2: dir = f3{u, 1.0f, v}; break;
            case 3: dir = f3{u, -1.0f, -v}; break;
            case 4: dir = f3{u, -v, 1.0f}; break;
            default: dir = f3{-u, -v, -1.0f};
        }
        dir = normalize3_q(dir);
        const f4 L = sample_cube_level_any(tb, cubemaps, cubemapCount, cubemap, dir, 0.0f);
        const float c0 = 0.28209479f, c1 = 0.48860251f, c2 = 1.09254843f, c3 = 0.31539157f, c4 = 0.54627422f;
        float sh[9];
        sh[0] = c0; sh[1] = c1 * dir.y; sh[2] = c1 * dir.z; sh[3] = c1 * dir.x;
        sh[4] = c2 * dir.x * dir.y; sh[5] = c2 * dir.y * dir.z; sh[6] = c3 * (3.0f * dir.z * dir.z - 1.0f); sh[7] = c2 * dir.z * dir.x;
        sh[8] = c4 * (dir.x * dir.x - dir.y * dir.y);
#pragma unroll
        for (int i = 0; i < 9; i++) {      // (int)(contrib * SH_FLOAT_SCALE): toward zero, saturating, NaN -> 0 (v_cvt_i32_f32)
            acc[3 * i] = (uint32_t)to_int_sat(L.x * sh[i] * (float)BRMI_SH_FLOAT_SCALE);
            acc[3 * i + 1] = (uint32_t)to_int_sat(L.y * sh[i] * (float)BRMI_SH_FLOAT_SCALE);
            acc[3 * i + 2] = (uint32_t)to_int_sat(L.z * sh[i] * (float)BRMI_SH_FLOAT_SCALE);
        }
    }
    // across the wave (lanes outside the face hold zeros), then across the four waves, then 27 atomics
#pragma unroll
    for (int k = 0; k < 27; k++) {
        uint32_t s = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o);
        acc[k] = s;
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < 27; k++) partial[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 27u) {
        const uint32_t s = ((partial[0][threadIdx.x] + partial[1][threadIdx.x]) + partial[2][threadIdx.x]) + partial[3][threadIdx.x];
        if (s != 0u) atomicAdd(reinterpret_cast<uint32_t*>(env->sphericalHarmonics) + threadIdx.x, s);
    }
}

// ================================================ blurEnvironment ================================================
struct PrefilterArgs { const brmi_texture_desc* source; const brmi_texture_desc* prefiltered; uint32_t size, levels; };
BRMI_DEV uint32_t reverse_bits(uint32_t b) {
    b = (b << 16) | (b >> 16);
    b = ((b & 0x55555555u) << 1) | ((b & 0xAAAAAAAAu) >> 1);
    b = ((b & 0x33333333u) << 2) | ((b & 0xCCCCCCCCu) >> 2);
    b = ((b & 0x0F0F0F0Fu) << 4) | ((b & 0xF0F0F0F0u) >> 4);
    b = ((b & 0x00FF00FFu) << 8) | ((b & 0xFF00FF00u) >> 8);
    return b;
}
BRMI_DEV uint32_t prefilter_tiles(uint32_t size, uint32_t level) { const uint32_t s = size >> level ? size >> level : 1u; return (s + 15u) / 16u; }
__global__ void __launch_bounds__(256) k_env_prefilter(PrefilterArgs a) {
    __shared__ float texelTables[256];
    __shared__ float halfVectors[16][3];      // ImportanceSampleGGX's H in tangent space, per Hammersley point of this workgroup's level
    // the workgroup's (level, face, tile): levels one after the other, six faces of tiles x tiles each
    uint32_t level = 0u, first = 0u;
    for (; level + 1u < a.levels; level++) {
        const uint32_t t = prefilter_tiles(a.size, level), n = t * t * 6u;
        if (blockIdx.x < first + n) break;
        first += n;
    }
    const uint32_t tiles = prefilter_tiles(a.size, level), local = blockIdx.x - first;
    const uint32_t face = local / (tiles * tiles), tile = local - face * tiles * tiles;
    const uint32_t sizeM = a.size >> level ? a.size >> level : 1u;
    stage_unorm_table(texelTables, threadIdx.x, 256u);
    if (threadIdx.x < 16u) {
        const float roughness = a.levels > 1u ? (float)level / (float)(a.levels - 1u) : 0.0f;
        const float al = roughness * roughness;
        const float xiX = (float)threadIdx.x / 16.0f, xiY = (float)reverse_bits(threadIdx.x) * 2.3283064365386963e-10f;
        const float phi = 2.0f * kPi * xiX;
        const float cosTheta = sqrtf((1.0f - xiY) / (1.0f + (al * al - 1.0f) * xiY));
        const float sinTheta = sqrtf(max2(0.0f, 1.0f - cosTheta * cosTheta));
        halfVectors[threadIdx.x][0] = cosf(phi) * sinTheta; halfVectors[threadIdx.x][1] = sinf(phi) * sinTheta; halfVectors[threadIdx.x][2] = cosTheta;
    }
    __syncthreads();
    TexelTables tb; tb.t = texelTables;
    uint32_t x, y; tile_texel(tile % tiles, tile / tiles, x, y);
    if (face >= 6u || x >= sizeM || y >= sizeM) return;
    const float u = ((float)x + 0.5f) / (float)sizeM * 2.0f - 1.0f, v = -(((float)y + 0.5f) / (float)sizeM * 2.0f - 1.0f);
    const f3 N = normalize3_q(face_uv_to_dir(face, u, v)), V = N;
    const f3 up = fabsf(N.z) < 0.999f ? f3{0.0f, 0.0f, 1.0f} : f3{1.0f, 0.0f, 0.0f};
    const f3 T = normalize3_q(cross3(up, N)), B = cross3(N, T);
    f3 sum{0.0f, 0.0f, 0.0f};
    float total = 0.0f;
#pragma nounroll
    for (uint32_t i = 0; i < 16u; i++) {
        const float hx = halfVectors[i][0], hy = halfVectors[i][1], hz = halfVectors[i][2];
        const f3 H = normalize3_q((T * hx + B * hy) + N * hz);
        const f3 L = normalize3_q((2.0f * dot3(V, H)) * H - V);
        const float ndotl = max2(dot3(N, L), 0.0f);
        if (ndotl > 0.0f) {
            const f4 c = sample_cube_level_any(tb, a.source, 1u, 0u, L, 0.0f);
            sum = sum + f3{c.x, c.y, c.z} * ndotl;
            total = total + ndotl;
        }
    }
    const f3 r = total > 0.0f ? sum / total : f3{0.0f, 0.0f, 0.0f};
    uint8_t* texels; size_t index;
    if (!dst_texel(kconst(a.prefiltered + face), BRMI_TEXTURE_FORMAT_RGBA8_UNORM, level, x, y, texels, index)) return;
    reinterpret_cast<uint32_t*>(texels)[index] = unorm8(r.x) | (unorm8(r.y) << 8) | (unorm8(r.z) << 16) | 0xFF000000u;
}

// brmi_debug_env_lookup: the lookup the kernels above and k_skybox call, one lane per sample
__global__ void __launch_bounds__(256) k_debug_env_lookup(const brmi_texture_desc* cubemaps, uint32_t cubemapCount, uint32_t cubemap, const float* dirs, const float* lods, float4* out, uint32_t n) {
    __shared__ float texelTables[256];
    stage_unorm_table(texelTables, threadIdx.x, 256u); __syncthreads();
    TexelTables tb; tb.t = texelTables;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f4 r = sample_cube_level_any(tb, cubemaps, cubemapCount, cubemap, f3{dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]}, lods[i]);
    out[i] = make_float4(r.x, r.y, r.z, r.w);
}

static int launched() { return hipGetLastError() == hipSuccess ? BRMI_OK : BRMI_ERR_HIP; }
int launch_env_convert(const brmi_texture_desc* equirect, const brmi_texture_desc* cube, uint32_t size, hipStream_t s) {
    const uint32_t t = (size + 15u) / 16u;
    hipLaunchKernelGGL(k_env_convert, dim3(t, t, 6), dim3(256), 0, s, equirect, cube, size);
    return launched();
}
int launch_env_project_sh(const brmi_texture_desc* cubemaps, uint32_t cubemapCount, brmi_environment_info* env, uint32_t size, hipStream_t s) {
    const float scale = 4.0f * 3.141592654f / (float)(size * size * 6u);      // Environment.cpp:31
    hipLaunchKernelGGL(k_env_sh_reset, dim3(1), dim3(64), 0, s, env, scale);
    const uint32_t t = (size + 15u) / 16u;
    hipLaunchKernelGGL(k_env_project_sh, dim3(t, t, 6), dim3(256), 0, s, cubemaps, cubemapCount, env, size);
    return launched();
}
int launch_env_prefilter(const brmi_texture_desc* source, const brmi_texture_desc* prefiltered, uint32_t size, uint32_t levels, hipStream_t s) {
    uint32_t blocks = 0u;
    for (uint32_t m = 0; m < levels; m++) { const uint32_t sz = std::max(1u, size >> m), t = (sz + 15u) / 16u; blocks += t * t * 6u; }
    hipLaunchKernelGGL(k_env_prefilter, dim3(blocks), dim3(256), 0, s, PrefilterArgs{source, prefiltered, size, levels});
    return launched();
}
int launch_debug_env_lookup(const brmi_texture_desc* cubemaps, uint32_t cubemapCount, uint32_t cubemap, const float* dirs, const float* lods, float* outRGBA, uint32_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_debug_env_lookup, dim3((n + 255u) / 256u), dim3(256), 0, s, cubemaps, cubemapCount, cubemap, dirs, lods, reinterpret_cast<float4*>(outRGBA), n);
    return launched();
}

}  // namespace brmi
