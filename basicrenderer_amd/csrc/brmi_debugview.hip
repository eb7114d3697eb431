// brmi_debugview.hip -- perFrame.outputType: the debug payload of the frame and its resolve to colour.
//
// Restates the debug writes of BR/shaders/gbuffer.hlsl:63-111 and BR/shaders/deferred.hlsl:65-103 (format: Include/debugPayload.hlsli) and
// PostProcessing/debugResolve.hlsl:50-106 as two full-screen passes BEHIND the frame: every input is a surface the frame has already produced (keys,
// visible-cluster list, depth, G-buffer planes, light clusters), so neither k_gbuffer nor k_shade knows about the mode.  The price: the
// material modes pack what the planes hold -- the values after the G-buffer formats quantised them -- where the reference packs the material inputs.
#include "brmi_internal.h"

namespace brmi {

constexpr unsigned long long kSentinel = 0xFFFFFFFFFFFFFFFFull;      // DEBUG_SENTINEL in both words: "no debug data" (the reference's graph clears to it)

struct DebugViewArgs {
    const unsigned long long* vis; const float* depth; const float* normals; const uint32_t* albedo; const unsigned long long* emissive;
    const uint32_t* metallicRoughness; const uint32_t* motion;
    const uint8_t* aoTerm;            // XeGTAO's final term where brmi_set_gtao bound one (mode AO packs the minimum the shading pass takes), else null
    const uint4* clusters; const ClusterSetup* setup; const uint32_t* counters; uint32_t clusterCapacity;
    const brmi_light_cluster* lightClusters; ShadeTables tables; const FrameSnapshot* snapshot;
    unsigned long long* payload;      // uint2 per pixel (x in the low word), tiled like the surfaces
    uint32_t* image;                  // rgba8, ROW-MAJOR W x H
    uint32_t W, H, tilesX, bandY0, bandY1; uint64_t firstPixel, pixelCount;
};

typedef float v4f __attribute__((ext_vector_type(4)));

BRMI_DEV unsigned long long pack_debug_float3(float x, float y, float z) {      // PackDebugFloat3: three RNE halves in x low, x high, y low
    return (unsigned long long)(f32_to_f16_bits(x) | (f32_to_f16_bits(y) << 16)) | ((unsigned long long)f32_to_f16_bits(z) << 32);
}
BRMI_DEV unsigned long long pack_debug_uint(uint32_t v) { return (unsigned long long)v; }      // PackDebugUint: (v, 0)

// The wave's tile (k_gbuffer's walk): `jb` = first pixel of the tile relative to firstPixel, wave-uniform; the lane is one pixel of the 8x8 tile
BRMI_DEV bool debug_in_band(const DebugViewArgs& a, uint64_t jb, uint32_t lane, uint32_t& px, uint32_t& py) {
    const uint32_t tile = (uint32_t)((a.firstPixel + jb) >> 6);
    px = (tile % a.tilesX) * 8u + (lane >> 3); py = (tile / a.tilesX) * 8u + (lane & 7u);
    return jb + lane < a.pixelCount && px < a.W && py < a.H && py >= a.bandY0 && py < a.bandY1;
}

// One instantiation per outputType: a launch reads the planes of ITS mode and nothing else.
template <int MODE>
__global__ void __launch_bounds__(256) k_debug_payload(DebugViewArgs a) {
    constexpr bool kKeyed = MODE == BRMI_OUTPUT_MESHLETS || MODE == BRMI_OUTPUT_GEOMETRY_GROUP;
    constexpr bool kLights = MODE == BRMI_OUTPUT_LIGHT_CLUSTER_ID || MODE == BRMI_OUTPUT_LIGHT_CLUSTER_LIGHT_COUNT;
    const uint64_t end = (a.pixelCount + 63ull) & ~63ull, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waveFirst = (uint64_t)blockIdx.x * blockDim.x + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
    uint32_t clusterCount = 0u;
    if (kKeyed) clusterCount = min(a.counters[CNT_VISIBLE] + a.counters[CNT_VISIBLE2], a.clusterCapacity);
    // modes 12 / 13: the third column of projectionInverse (the view depth's dot product) and the grid, from the frame's own snapshot as k_shade has them
    float ip02 = 0.0f, ip12 = 0.0f, ip22 = 0.0f, ip32 = 0.0f; uint32_t gx = 0u, gy = 0u, gz = 0u;
    if (kLights) {
        const auto* cam = kconst(&a.snapshot->camera); const auto* pf = kconst(&a.snapshot->perFrame);
        ip02 = cam->projectionInverse[0][2]; ip12 = cam->projectionInverse[1][2]; ip22 = cam->projectionInverse[2][2]; ip32 = cam->projectionInverse[3][2];
        gx = pf->lightClusterGridSizeX; gy = pf->lightClusterGridSizeY; gz = pf->lightClusterGridSizeZ;
    }
    for (uint64_t jb = waveFirst; jb < end; jb += stride) {
        uint32_t px, py;
        if (!debug_in_band(a, jb, lane, px, py)) continue;
        const uint64_t i = a.firstPixel + jb + lane;
        unsigned long long out = kSentinel;
        if (kKeyed) {
            const unsigned long long key = __builtin_nontemporal_load(a.vis + i);
            const uint32_t triId = (uint32_t)(key & 0x7Full), clusterIndex = (uint32_t)((key >> BRMI_VIS_TRI_BITS) & 0x3FFFFFFull);
            // a key that names no cluster of the frame's list, or no triangle of the cluster, is empty (k_gbuffer's rule)
            if (key != BRMI_VIS_EMPTY && clusterIndex < clusterCount && triId < ((a.setup[clusterIndex].counts >> 8) & 0xFFu)) {
                const uint4* c = a.clusters + clusterIndex;
                uint4 rec = make_uint4(0u, c->y, 0u, 0u);
                if (MODE == BRMI_OUTPUT_GEOMETRY_GROUP) rec.z = c->z;
                out = pack_debug_uint(MODE == BRMI_OUTPUT_MESHLETS ? vc_meshlet(rec) : vc_group(rec));
            }
        } else {
            const float d = __builtin_nontemporal_load(a.depth + i);
            if (as_u32(d) != BRMI_DEPTH_EMPTY_BITS) {
                if (MODE == BRMI_OUTPUT_NORMAL) {
                    const v4f n = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(a.normals) + i);
                    out = pack_debug_float3(n.x * 0.5f + 0.5f, n.y * 0.5f + 0.5f, n.z * 0.5f + 0.5f);
                } else if (MODE == BRMI_OUTPUT_ALBEDO) {
                    const uint32_t al = __builtin_nontemporal_load(a.albedo + i);
                    out = pack_debug_float3(unorm8_to_f32(al), unorm8_to_f32(al >> 8), unorm8_to_f32(al >> 16));
                } else if (MODE == BRMI_OUTPUT_AO) {
                    uint32_t code = __builtin_nontemporal_load(a.albedo + i) >> 24;
                    if (a.aoTerm) code = min(code, (uint32_t)a.aoTerm[i]);      // (wave-uniform test)
                    const float ao = unorm8_to_f32(code);
                    out = pack_debug_float3(ao, ao, ao);
                } else if (MODE == BRMI_OUTPUT_METALLIC || MODE == BRMI_OUTPUT_ROUGHNESS) {
                    const float v = unorm8_to_f32(__builtin_nontemporal_load(a.metallicRoughness + i) >> (MODE == BRMI_OUTPUT_ROUGHNESS ? 8 : 0));
                    out = pack_debug_float3(v, v, v);
                } else if (MODE == BRMI_OUTPUT_EMISSIVE) {
                    const unsigned long long e = __builtin_nontemporal_load(a.emissive + i);
                    out = pack_debug_float3(f16_bits_to_f32((uint32_t)e & 0xFFFFu), f16_bits_to_f32((uint32_t)(e >> 16) & 0xFFFFu), f16_bits_to_f32((uint32_t)(e >> 32) & 0xFFFFu));
                } else if (MODE == BRMI_OUTPUT_DEPTH) {
                    // the shader rounds the product to fp32 and f32tof16 rounds that again; left to itself the compiler selects v_fma_mixlo_f16 for
                    // "multiply, then convert", which rounds the exact product ONCE (one half ulp off on a pixel in 10^4): keep the product a value of its own
                    float s = fabsf(d) * 0.1f;
                    asm volatile("" : "+v"(s));
                    out = pack_debug_float3(s, s, s);
                } else if (MODE == BRMI_OUTPUT_MOTION_VECTORS) {
                    const uint32_t mv = __builtin_nontemporal_load(a.motion + i);
                    out = pack_debug_float3(f16_bits_to_f32(mv & 0xFFFFu) * 0.5f + 0.5f, f16_bits_to_f32(mv >> 16) * 0.5f + 0.5f, 0.5f);
                } else if (kLights) {
                    // the view depth k_shade feeds its slice lookup: |(clipPos . projectionInverse).z * depth|, clipPos = (uv * 2 - 1, 1, 1), uv.y flipped
                    const AxisEntry ax = a.tables.x[px], ay = a.tables.y[py];
                    const float cx = ax.uv * 2.0f - 1.0f, cy = (1.0f - ay.uv) * 2.0f - 1.0f;
                    const float z = fabsf((((cx * ip02 + cy * ip12) + ip22) + ip32) * d);
                    // its slice from the exact slice starts (brmi_update): the last slice that starts at or before z; the table ends at gz, the first
                    // slice behind the grid
                    const auto* start = kconst(a.tables.sliceStart);
                    uint32_t e = 0u;
                    for (uint32_t s = 1u; s <= gz; s++) e += (z >= start[s]) ? 1u : 0u;
                    if (MODE == BRMI_OUTPUT_LIGHT_CLUSTER_ID) out = pack_debug_uint(e);      // (lighting.hlsli:509: clusterID.z, not the flat index)
                    else {
                        const uint32_t ci = (uint32_t)((float)ax.tile + (float)ay.tile * (float)gx + (float)e * (float)gx * (float)gy);
                        out = pack_debug_uint(ci < gx * gy * gz ? a.lightClusters[ci].numLights : 0u);      // (behind the grid: no cluster, no lights)
                    }
                }
            }
        }
        __builtin_nontemporal_store(out, a.payload + i);
    }
}

BRMI_DEV uint32_t srgb_code(float c) {      // LinearToSRGB = pow(c, 1 / 2.2), then (uint)(sat(x) * 255 + 0.5); negative and NaN give 0
    return (uint32_t)(sat(powf(c, 1.0f / 2.2f)) * 255.0f + 0.5f);
}

// debugResolve.hlsl:50-106 at render resolution.  HASHED: the payload is an integer coloured by HashToColor, otherwise three halves.
template <bool HASHED>
__global__ void __launch_bounds__(256) k_debug_resolve(DebugViewArgs a) {
    const uint64_t end = (a.pixelCount + 63ull) & ~63ull, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waveFirst = (uint64_t)blockIdx.x * blockDim.x + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
    for (uint64_t jb = waveFirst; jb < end; jb += stride) {
        uint32_t px, py;
        if (!debug_in_band(a, jb, lane, px, py)) continue;
        const unsigned long long p = __builtin_nontemporal_load(a.payload + a.firstPixel + jb + lane);
        if (p == kSentinel) continue;      // the reference discards: the caller's image shows through
        float r, g, b;
        if (HASHED) {
            uint32_t h = (uint32_t)p;      // HashToColor, debugPayload.hlsli:70-82
            h = ((h >> 16) ^ h) * 0x45d9f3bu;
            h = ((h >> 16) ^ h) * 0x45d9f3bu;
            h = (h >> 16) ^ h;
            r = unorm8_to_f32(h); g = unorm8_to_f32(h >> 8); b = unorm8_to_f32(h >> 16);
        } else {
            r = f16_bits_to_f32((uint32_t)p & 0xFFFFu); g = f16_bits_to_f32((uint32_t)(p >> 16) & 0xFFFFu); b = f16_bits_to_f32((uint32_t)(p >> 32) & 0xFFFFu);
        }
        a.image[(uint64_t)py * a.W + px] = srgb_code(r) | (srgb_code(g) << 8) | (srgb_code(b) << 16) | 0xFF000000u;
    }
}

bool debug_view_mode_built(uint32_t mode) {
    switch (mode) {
        case BRMI_OUTPUT_NORMAL: case BRMI_OUTPUT_ALBEDO: case BRMI_OUTPUT_METALLIC: case BRMI_OUTPUT_ROUGHNESS: case BRMI_OUTPUT_EMISSIVE: case BRMI_OUTPUT_AO:
        case BRMI_OUTPUT_DEPTH: case BRMI_OUTPUT_MESHLETS: case BRMI_OUTPUT_LIGHT_CLUSTER_ID: case BRMI_OUTPUT_LIGHT_CLUSTER_LIGHT_COUNT:
        case BRMI_OUTPUT_MOTION_VECTORS: case BRMI_OUTPUT_GEOMETRY_GROUP: return true;
        default: return false;
    }
}

// The payload of p->pfHost.outputType (the caller has checked the mode and the binding), then its resolve where an image is bound.
int launch_debug_view(brmi_pass* p, hipStream_t s) {
    if (int rc = ensure_frame_constants(p, s)) return rc;
    DebugViewArgs a;
    a.vis = static_cast<const unsigned long long*>(p->res[BRMI_RES_VISIBILITY]); a.depth = static_cast<const float*>(p->res[BRMI_RES_LINEAR_DEPTH]);
    a.normals = static_cast<const float*>(p->res[BRMI_RES_GBUF_NORMALS]); a.albedo = static_cast<const uint32_t*>(p->res[BRMI_RES_GBUF_ALBEDO]);
    a.emissive = static_cast<const unsigned long long*>(p->res[BRMI_RES_GBUF_EMISSIVE]); a.metallicRoughness = static_cast<const uint32_t*>(p->res[BRMI_RES_GBUF_METALLIC_ROUGHNESS]);
    a.motion = static_cast<const uint32_t*>(p->res[BRMI_RES_GBUF_MOTION_VECTORS]);
    a.aoTerm = p->gtao.on ? static_cast<const uint8_t*>(p->gtao.b.aoTerm) : nullptr;
    a.clusters = static_cast<const uint4*>(p->res[BRMI_RES_VISIBLE_CLUSTERS]); a.setup = p->wsPtr<ClusterSetup>(p->ws.clusterSetup); a.counters = p->counters();
    a.clusterCapacity = p->cfg.maxVisibleClusters;
    a.lightClusters = static_cast<const brmi_light_cluster*>(p->res[BRMI_RES_LIGHT_CLUSTERS]); a.tables = shade_tables_of(p); a.snapshot = p->wsPtr<FrameSnapshot>(p->ws.frameSnapshot);
    a.payload = static_cast<unsigned long long*>(p->debugView.b.payload); a.image = static_cast<uint32_t*>(p->debugView.b.image);
    a.W = p->cfg.width; a.H = p->cfg.height; a.tilesX = p->tilesX; a.bandY0 = p->bandY0; a.bandY1 = p->bandY1; a.firstPixel = p->bandFirstPixel; a.pixelCount = p->bandPixelCount;
    const uint32_t mode = p->pfHost.outputType;
    const dim3 grid((uint32_t)std::min<uint64_t>(std::max<uint64_t>((a.pixelCount + 255u) / 256u, 1u), 8192u));
    switch (mode) {
#define BRMI_DV_CASE(M) case M: hipLaunchKernelGGL(k_debug_payload<M>, grid, dim3(256), 0, s, a); break
        BRMI_DV_CASE(BRMI_OUTPUT_NORMAL); BRMI_DV_CASE(BRMI_OUTPUT_ALBEDO); BRMI_DV_CASE(BRMI_OUTPUT_METALLIC); BRMI_DV_CASE(BRMI_OUTPUT_ROUGHNESS);
        BRMI_DV_CASE(BRMI_OUTPUT_EMISSIVE); BRMI_DV_CASE(BRMI_OUTPUT_AO); BRMI_DV_CASE(BRMI_OUTPUT_DEPTH); BRMI_DV_CASE(BRMI_OUTPUT_MESHLETS);
        BRMI_DV_CASE(BRMI_OUTPUT_LIGHT_CLUSTER_ID); BRMI_DV_CASE(BRMI_OUTPUT_LIGHT_CLUSTER_LIGHT_COUNT); BRMI_DV_CASE(BRMI_OUTPUT_MOTION_VECTORS);
        BRMI_DV_CASE(BRMI_OUTPUT_GEOMETRY_GROUP);
#undef BRMI_DV_CASE
        default: return fail(p, BRMI_ERR_INVALID, "brmi_debug_view: outputType %u has no payload kernel", mode);
    }
    BRMI_LAUNCH_CHECK(p, "k_debug_payload");
    if (a.image) {
        const bool hashed = mode == BRMI_OUTPUT_MESHLETS || mode == BRMI_OUTPUT_GEOMETRY_GROUP || mode == BRMI_OUTPUT_LIGHT_CLUSTER_ID || mode == BRMI_OUTPUT_LIGHT_CLUSTER_LIGHT_COUNT;
        if (hashed) hipLaunchKernelGGL(k_debug_resolve<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(k_debug_resolve<false>, grid, dim3(256), 0, s, a);
        BRMI_LAUNCH_CHECK(p, "k_debug_resolve");
    }
    return BRMI_OK;
}

}  // namespace brmi
