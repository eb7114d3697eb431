// brmi_skybox.hip -- the sky behind the frame: SkyboxRenderPass for gfx950.
//
// Reference: BR/shaders/skybox.hlsl (the primary pass is Deferred -> Skybox -> Forward, and this pass writes the lit HDR target).
// MI355X-first differences: one wave is one 8x8 tile of the surfaces' tiled layout (the depth read and both writes are contiguous per wave); the tile is
// tested with one ballot and a tile without an empty pixel ends before the camera is loaded; camera and environment words come through scalar loads from the
// frame's own snapshot (a split frame shades while the caller rewrites its camera buffer).
// Arithmetic: skybox.hlsl line by line in IEEE fp32 without contraction; mul(v, M) and dot as brmi_device.h states them, normalize = normalize3_q.
#include <algorithm>

#include "brmi_internal.h"
#include "brmi_texture.h"

namespace brmi {

struct SkyboxArgs {
    const float* depth; unsigned long long* hdr; uint32_t* motion;
    const FrameSnapshot* snapshot; ShadeTables tables;
    const brmi_environment_info* environments; uint32_t environmentCount; const brmi_texture_desc* cubemaps; uint32_t cubemapCount;
    uint32_t W, H, tilesX, bandY0, bandY1; uint64_t firstPixel, pixelCount;
};

BRMI_DEV float keep(float x) { asm volatile("" : "+v"(x)); return x; }      // (a value of its own in front of its fp16 conversion: no v_fma_mix)
typedef const __attribute__((address_space(4))) float* KFloats;
BRMI_DEV m4 load_m4_uniform(KFloats q) {      // sixteen words through the scalar path
    m4 r;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) r.m[i][j] = q[i * 4 + j];
    return r;
}

__global__ void __launch_bounds__(256) k_skybox(SkyboxArgs a) {
    __shared__ float texelTables[4][256];      // the UNORM decode table (an RGBA8 sky cube), per wave, filled by the wave's first tile that has sky in it: a frame full of geometry stages nothing
    bool staged = false;
    TexelTables tb; tb.t = texelTables[threadIdx.x >> 6];
    const uint64_t end = (a.pixelCount + 63ull) & ~63ull, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waveFirst = (uint64_t)blockIdx.x * blockDim.x + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
    for (uint64_t jb = waveFirst; jb < end; jb += stride) {
        const uint32_t tile = (uint32_t)((a.firstPixel + jb) >> 6);
        const uint32_t px = (tile % a.tilesX) * 8u + (lane >> 3), py = (tile / a.tilesX) * 8u + (lane & 7u);
        const bool inBand = jb + lane < a.pixelCount && px < a.W && py < a.H && py >= a.bandY0 && py < a.bandY1;
        const uint64_t i = a.firstPixel + jb + lane;
        const bool empty = inBand && as_u32(__builtin_nontemporal_load(a.depth + i)) == BRMI_DEPTH_EMPTY_BITS;
        if (__ballot(empty) == 0ull) continue;      // (nearly every tile of a frame full of geometry)
        const auto* cam = kconst(&a.snapshot->camera);
        const uint32_t envIndex = kconst(&a.snapshot->perFrame)->activeEnvironmentIndex;
        const uint32_t cubemap = envIndex < a.environmentCount ? kconst(a.environments + envIndex)->cubeMapDescriptorIndex : 0xFFFFFFFFu;
        if (!staged) { stage_unorm_table(texelTables[threadIdx.x >> 6], lane, 64u); wave_lds_sync(); staged = true; }
        if (!empty) continue;
        const float uvx = a.tables.x[px].uv, uvy = 1.0f - a.tables.y[py].uv;      // (pixel + 0.5) / screenRes, as the shading pass reads them (the frame's row under the interleaved partition)
        const float nx = uvx * 2.0f - 1.0f, ny = uvy * 2.0f - 1.0f;
        const f4 viewDirH = mul_vm(f4{nx, ny, 1.0f, 1.0f}, load_m4_uniform(&cam->projectionInverse[0][0]));
        const float w = max2(fabsf(viewDirH.w), 1e-6f);
        const f3 viewDir = normalize3_q(f3{viewDirH.x / w, viewDirH.y / w, viewDirH.z / w});
        const f3 worldDir = normalize3_q(xyz(mul_vm(f4{viewDir.x, viewDir.y, viewDir.z, 0.0f}, load_m4_uniform(&cam->viewInverse[0][0]))));
        const f3 curView = normalize3_q(xyz(mul_vm(f4{worldDir.x, worldDir.y, worldDir.z, 0.0f}, load_m4_uniform(&cam->view[0][0]))));
        const f4 curClip = mul_vm(f4{curView.x, curView.y, curView.z, 1.0f}, load_m4_uniform(&cam->unjitteredProjection[0][0]));
        const float cw = max2(fabsf(curClip.w), 1e-6f);
        const f3 prevView = normalize3_q(xyz(mul_vm(f4{worldDir.x, worldDir.y, worldDir.z, 0.0f}, load_m4_uniform(&cam->prevView[0][0]))));
        const f4 prevClip = mul_vm(f4{prevView.x, prevView.y, prevView.z, 1.0f}, load_m4_uniform(&cam->prevUnjitteredProjection[0][0]));
        const float pw = max2(fabsf(prevClip.w), 1e-6f);
        const float mvx = curClip.x / cw - prevClip.x / pw, mvy = curClip.y / cw - prevClip.y / pw;
        const f4 c = sample_cube_level_any(tb, a.cubemaps, a.cubemapCount, cubemap, worldDir, 0.0f);
        __builtin_nontemporal_store((unsigned long long)pack_half4(keep(c.x), keep(c.y), keep(c.z), 1.0f), a.hdr + i);
        __builtin_nontemporal_store(f32_to_f16_bits(keep(mvx)) | (f32_to_f16_bits(keep(mvy)) << 16), a.motion + i);
    }
}

int launch_skybox(brmi_pass* p, hipStream_t s) {
    if (int rc = ensure_frame_constants(p, s)) return rc;
    SkyboxArgs a;
    a.depth = static_cast<const float*>(p->res[BRMI_RES_LINEAR_DEPTH]); a.hdr = static_cast<unsigned long long*>(p->res[BRMI_RES_HDR_COLOR]);
    a.motion = static_cast<uint32_t*>(p->res[BRMI_RES_GBUF_MOTION_VECTORS]);
    a.snapshot = p->wsPtr<FrameSnapshot>(p->ws.frameSnapshot); a.tables = shade_tables_of(p);
    a.environments = p->env.b.environments; a.environmentCount = p->env.b.environmentCount; a.cubemaps = p->env.b.cubemaps; a.cubemapCount = p->env.b.cubemapCount;
    a.W = p->cfg.width; a.H = p->cfg.height; a.tilesX = p->tilesX; a.bandY0 = p->bandY0; a.bandY1 = p->bandY1; a.firstPixel = p->bandFirstPixel; a.pixelCount = p->bandPixelCount;
    const dim3 grid((uint32_t)std::min<uint64_t>(std::max<uint64_t>((a.pixelCount + 255u) / 256u, 1u), 8192u));
    hipLaunchKernelGGL(k_skybox, grid, dim3(256), 0, s, a);
    BRMI_LAUNCH_CHECK(p, "k_skybox");
    return BRMI_OK;
}

}  // namespace brmi
