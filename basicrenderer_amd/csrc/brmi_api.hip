// brmi_api.hip -- the C ABI of libbrmi.so (include/brmi.h): pass lifecycle and stage scheduling.
//
// Host side of the drop-in.  Mirrors the five phases of the reference's ComputePass /
// IRenderGraphExtension (DeclareResourceUsages / Setup / Update / Execute / Cleanup) and the order
// in which CLodExtension + RenderGraphBuildHelper schedule the chain
// (BR/src/Render/GraphExtensions/CLodExtension.cpp:1580-2088, BR/include/Render/RenderGraphBuildHelper.h:220-414).
// The library never allocates device memory: the graph (caller) owns every resource, exactly as
// in the reference; kernels are enqueued on the caller's stream and nothing here synchronises
// except the explicit read-back calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "brmi_device.h"
#include "brmi_display_math.h"
#include "brmi_internal.h"

namespace brmi {

__global__ void k_debug_arith(const float* a, const float* b, float* outDiv, float* outSqrt, uint32_t* outHalf, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    outDiv[i] = a[i] / b[i];
    outSqrt[i] = sqrtf(fabsf(a[i]));
    outHalf[i] = f32_to_f16_bits(a[i]);
}

__global__ void k_debug_arith_in_range(const float* a, float* outRcp, float* outSqrt, float* outNorm, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = a[i];
    outRcp[i] = in_range_pow63(x) ? rcp_rn_in_range(x) : 1.0f / x;
    outSqrt[i] = in_range_pow63(x) ? sqrt_rn_in_range(x) : sqrtf(x);
    float len; const f3 v = normalize3_len(f3{x, 1.0f, 0.5f}, x, len);      // the guarded pair on the same operand
    outNorm[i] = v.y;                                                        // = 1 / sqrt(x)
}

int fail(brmi_pass* p, int code, const char* fmt, ...) {
    std::string msg;
    va_list ap; va_start(ap, fmt); vrefuse(msg, code, fmt, ap); va_end(ap);
    if (p) p->err = msg;
    return code;
}

static uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

static const char* kResNames[BRMI_RES_COUNT] = {
    "Builtin::PrimaryCamera::VisibilityTexture", "Builtin::PrimaryCamera::LinearDepthMap", "Builtin::GBuffer::Normals", "Builtin::GBuffer::Albedo",
    "Builtin::GBuffer::Coat", "Builtin::GBuffer::Emissive", "Builtin::GBuffer::Fuzz", "Builtin::GBuffer::MetallicRoughness", "Builtin::GBuffer::MotionVectors",
    "Builtin::Color::HDRColorTarget", "Builtin::CLod::VisibleClusters", "Builtin::Light::ClusterBuffer", "Builtin::Light::PagesBuffer",
    "Builtin::PrimaryCamera::LinearDepthMap(mips)", "brmi::Workspace"};
static const uint32_t kResBpp[BRMI_RES_COUNT] = {8, 4, 16, 4, 8, 8, 8, 4, 4, 8, 0, 0, 0, 4, 0};

static void compute_sizes(brmi_pass* p) {
    const brmi_config& c = p->cfg;
    p->tilesX = (c.width + 7) / 8; p->tilesY = (c.height + 7) / 8;
    p->paddedPixels = (uint64_t)p->tilesX * p->tilesY * 64;
    p->bandY0 = c.bandY0; p->bandY1 = (c.bandY1 == 0 || c.bandY1 > c.height) ? c.height : c.bandY1;
    if (p->bandY0 >= p->bandY1) p->bandY0 = 0;
    p->stripes = c.stripeCount > 1u ? StripeMap{c.stripeRows, c.stripeCount, c.stripeIndex, c.fullHeight} : StripeMap{0u, 0u, 0u, c.height};
    { const uint32_t t0 = p->bandY0 / 8, t1 = (p->bandY1 + 7) / 8; p->bandFirstPixel = (uint64_t)t0 * p->tilesX * 64; p->bandPixelCount = (uint64_t)(t1 - t0) * p->tilesX * 64; }
    p->numLightClusters = c.lightClusterSize[0] * c.lightClusterSize[1] * c.lightClusterSize[2];
    p->lightPagePool = p->numLightClusters * BRMI_LIGHT_PAGES_PER_CLUSTER;
    if (const long v = tuning("light_page_pool", 0)) p->lightPagePool = (uint32_t)std::max(1l, v);   // tests: exhaust the page pool
    for (int i = 0; i < BRMI_RES_COUNT; i++) p->resNeed[i] = 0;
    for (int i = BRMI_RES_VISIBILITY; i <= BRMI_RES_HDR_COLOR; i++) p->resNeed[i] = p->paddedPixels * kResBpp[i];
    p->resNeed[BRMI_RES_VISIBLE_CLUSTERS] = (uint64_t)c.maxVisibleClusters * 16;
    p->resNeed[BRMI_RES_LIGHT_CLUSTERS] = (uint64_t)p->numLightClusters * sizeof(brmi_light_cluster);
    p->resNeed[BRMI_RES_LIGHT_PAGES] = (uint64_t)p->lightPagePool * sizeof(brmi_light_page);
    // HZB: mip chain of the power-of-two padded linear depth (built only with occlusion culling)
    p->hzbMipOffsets.clear(); p->hzbMipW.clear(); p->hzbMipH.clear();
    uint64_t hzbFloats = 0;
    if (c.enableOcclusionCulling) {
        uint32_t w = 1, h = 1; while (w < c.width) w <<= 1; while (h < c.height) h <<= 1;
        for (uint32_t mip = 0;; mip++) {      // mip 0 is the depth map itself: no storage
            p->hzbMipOffsets.push_back(hzbFloats); p->hzbMipW.push_back(w); p->hzbMipH.push_back(h);
            if (mip > 0) hzbFloats += (uint64_t)w * h;
            if (w == 1 && h == 1) break;
            w = std::max(1u, w >> 1); h = std::max(1u, h >> 1);
        }
    }
    p->hzbMipCount = (uint32_t)p->hzbMipOffsets.size();
    p->resNeed[BRMI_RES_HZB] = std::max<uint64_t>(16, hzbFloats * 4);
    // workspace carve-up
    Workspace& w = p->ws; uint64_t off = 0;
    auto take = [&](uint64_t bytes) { uint64_t o = off; off = align_up(off + bytes, 256); return o; };
    // counters and both bitmasks are adjacent: one fill clears them at the start of a frame
    w.counters = take((uint64_t)(CNT_WORDS + 64) * 4);
    w.bitmask1 = take((uint64_t)p->totalWords * 4);
    w.bitmask2 = take((uint64_t)p->totalWords * 4);
    w.blockDirty = take((uint64_t)2 * (p->scanBlocks + 1));      // per phase and 2048-word block of the bitmask: some survivor set a bit there (the ranking skips the others)
    // phase 2's footprint for the second depth-chain build: a byte per 32 x 32 px block of the chain's head, from byte 4 (byte 0: "everything", stored by a triangle of more than 16 blocks)
    w.chainDirty = take(4ull + (uint64_t)((c.width + 31u) / 32u) * ((c.height + 31u) / 32u));
    w.frameClearBytes = off - w.counters;
    w.frontierA = take((uint64_t)c.maxTraversalRecords * sizeof(NodeRecord));
    w.frontierB = take((uint64_t)c.maxTraversalRecords * sizeof(NodeRecord));
    w.buckets = take((uint64_t)c.maxTraversalRecords * sizeof(BucketRecord));
    w.tempVisible = take((uint64_t)c.maxVisibleClusters * sizeof(TempVisible));
    w.wordPrefix = take((uint64_t)p->totalWords * 4);
    w.blockSums = take((uint64_t)(p->scanBlocks + 1) * 4);
    w.scanAgg = take(65 * 8);
    w.instanceBitBase = take((uint64_t)std::max<size_t>(1, p->tables.instanceBitBase.size()) * 4);
    w.segPrefix = take((uint64_t)std::max<size_t>(1, p->tables.segPrefix.size()) * 4);
    w.meshLevelWidth = take((uint64_t)std::max<size_t>(1, p->tables.meshLevelWidth.size()) * 4);
    w.flatNodes = take((uint64_t)std::max<size_t>(1, p->tables.flatNodes.size()) * sizeof(FlatNode));
    w.flatLeaves = take((uint64_t)std::max<size_t>(1, p->tables.flatLeaves.size()) * sizeof(FlatLeaf));
    w.instanceWalk = take((uint64_t)std::max<size_t>(1, p->tables.instanceWalk.size()) * sizeof(InstanceWalk));
    w.planes = take((uint64_t)2 * c.lightClusterSize[2] * 4);
    // phase-1 -> phase-2 hand-over (reference: clodStructs.hlsli:629-652); the replay bucket array doubles as the
    // phase-2 bucket array, so it has the full record capacity
    w.replayNodes = take(c.enableOcclusionCulling ? (uint64_t)c.maxTraversalRecords * sizeof(NodeRecord) : 16);
    w.replayBuckets = take(c.enableOcclusionCulling ? (uint64_t)c.maxTraversalRecords * sizeof(BucketRecord) : 16);
    w.lightVS = take((uint64_t)std::max(1u, p->scene.lightCount) * 16);
    w.lightMeta = take((uint64_t)std::max(1u, p->scene.lightCount) * 4);
    w.clusterPages = take((uint64_t)p->numLightClusters * 4);
    w.clusterHits = take((uint64_t)p->numLightClusters * 4);
    w.pageTotal = take(16);
    w.lightHitMasks = take((uint64_t)p->numLightClusters * ((std::max(1u, p->scene.lightCount) + 63u) / 64u) * 8);
    p->binsX = (c.width + 255) / 256; p->binsY = (c.height + 15) / 16;
    w.binCounts = take((uint64_t)p->binsX * p->binsY * 4 * BRMI_BIN_COUNT_STRIDE);
    w.binRecords = take((uint64_t)p->binsX * p->binsY * p->binCapacity * 64);
    w.binOverflow = take((uint64_t)CNT_STRIPE_COUNT * p->binOverflowPerStripe * 64);
    // the plan of a k_raster_bins launch: header, three words per bin, the (bin, slice) items; scratch tiles of 32 KB for the slices of bins
    // that several workgroups walk (2048 tiles = 64 MB: a 4K frame whose every bin is full would want 16 k; bins beyond merge with atomics)
    p->binItemCapacity = p->binsX * p->binsY * std::max(1u, (p->binCapacity + 31u) / 32u > 256u ? 256u : (p->binCapacity + 31u) / 32u);
    p->binItemCapacity = std::min<uint32_t>(p->binItemCapacity, 1u << 22);
    p->binScratchTiles = (uint32_t)std::max(0l, tuning("bin_scratch_tiles", p->binScratchTiles));
    w.binPlan = take((uint64_t)(16 + 3 * p->binsX * p->binsY) * 4);
    w.binItems = take((uint64_t)p->binItemCapacity * 4);
    w.binScratch = take((uint64_t)std::max(1u, p->binScratchTiles) * 4096 * 8);
    w.clusterSetup = take((uint64_t)c.maxVisibleClusters * sizeof(ClusterSetup));
    // resolve arena: full tables (72 B per vertex + triangle slot) for up to 2^20 clusters = 9.7 GB of the 288; a configuration
    // that allows more visible clusters keeps the per-pixel path for the clusters that do not fit
    p->resolveCapacity = (uint32_t)std::min<uint64_t>((uint64_t)c.maxVisibleClusters, 1ull << 20) * BRMI_MESHLET_MAX_TRIS;
    if (const long v = tuning("resolve_capacity", 0)) p->resolveCapacity = (uint32_t)std::max(1l, v);   // tests: force the per-pixel fallback
    w.resolveVerts = take((uint64_t)p->resolveCapacity * sizeof(ResolveVertex));
    w.resolveTris = take((uint64_t)p->resolveCapacity * sizeof(ResolveTriangle));
    w.shadeTables = take(((uint64_t)2 * c.width + 2 * c.height + 64) * 4);
    w.matWords = take((uint64_t)std::max(1u, p->scene.materialCount) * sizeof(MaterialWords));
    w.layerUniform = take(sizeof(LayerUniform));
    w.frameConst = take(4 * 64);      // three matrix products and (round 6) the band's two planes
    w.frameSnapshot = take(sizeof(FrameSnapshot));
    w.matConst = take((uint64_t)std::max(1u, p->scene.openpbrMaterialCount) * sizeof(MatConst));
    w.objConst = take((uint64_t)std::max(1u, p->scene.perObjectCount) * OBJ_CONST_FLOATS * 4);
    // (a band that may change from frame to frame: sized for the whole frame)
    p->deferredStripeCapacity = (uint32_t)((((c.dynamicBand ? p->paddedPixels : p->bandPixelCount) / 4096 + CNT_STRIPE_COUNT) / CNT_STRIPE_COUNT) * 4096);   // 64-tile runs of a stripe x 4096 pixels
    w.deferredPixels = take((uint64_t)3 * CNT_STRIPE_COUNT * p->deferredStripeCapacity * 4);      // one set of striped lists per layered class
    w.lutF = take((uint64_t)(32768 + 1024 + 1024 + 32 + 256) * 4);
    w.shadeRows = take((uint64_t)std::max(1u, p->scene.openpbrMaterialCount) * 256 * 512);    // (OpenPBR material, roughness code) -> folded energy-table rows of the shading pass
    w.shadeAvgs = take((uint64_t)std::max(1u, p->scene.openpbrMaterialCount) * 256 * 8);
    w.ggxQuads = take(256 * 48);                                                                  // roughness code -> the GGX albedo fit as quadratics in N.V
    w.shadeLights = take((uint64_t)std::max(1u, p->scene.lightCount) * 64);                     // the shading pass's 64 B record per active light
    w.clusterList = take((uint64_t)p->numLightClusters * 8);                                    // per light cluster: first entry / length of its flat light list
    w.listEntries = take((uint64_t)p->lightPagePool * BRMI_LIGHTS_PER_PAGE * 4 + 256);
    w.listRecords = take((uint64_t)p->lightPagePool * BRMI_LIGHTS_PER_PAGE * 64 + 4096);      // ... and the lights' 64 B shading records in the same order        // the page contents once more, in the order the page walk visits them
    // textured / alpha-tested scenes only: where each visible cluster's UV set lives, the texcoords of the resolve arena's vertices,
    // and the alpha-test operands that travel with binned triangles
    const bool uvs = p->tables.hasTextures || p->tables.hasAlphaTest || p->tables.hasVertexColors;
    w.clusterUv = take(uvs ? (uint64_t)c.maxVisibleClusters * 32 : 16);
    w.resolveColors = take(p->tables.hasVertexColors ? (uint64_t)p->resolveCapacity * 4 : 16);
    w.resolveUVs = take(p->tables.hasTextures ? (uint64_t)p->resolveCapacity * 8 * p->tables.uvSets : 16);
    w.binAlpha = take(p->tables.hasAlphaTest ? (uint64_t)p->binsX * p->binsY * p->binCapacity * 48 : 16);
    w.overflowAlpha = take(p->tables.hasAlphaTest ? (uint64_t)CNT_STRIPE_COUNT * p->binOverflowPerStripe * 48 : 16);
    w.alphaMats = take(p->tables.hasAlphaTest ? (uint64_t)std::max(1u, p->scene.materialCount) * 128 : 16);
    // round 6, the draw list: per-meshlet boxes of the resident pages, the (slab, page) -> first box table, and the three lists of a frame
    w.meshletBoxes = take((uint64_t)std::max(1u, p->tables.totalBoxes) * sizeof(MeshletBox));
    w.pageBoxBase = take((uint64_t)std::max<size_t>(1, p->tables.pageBoxBase.size()) * 4);
    w.pageRefs = take((uint64_t)std::max<size_t>(1, p->tables.pageRefs.size()) * sizeof(PageRef));
    w.drawList = take(p->holdEnabled ? (uint64_t)c.maxVisibleClusters * 4 : 16);
    w.generalList = take(p->leanMinClusters != 0u ? (uint64_t)c.maxVisibleClusters * 4 : 16);
    w.bigQueue = take(p->leanMinClusters != 0u ? (uint64_t)p->leanQueue * 96 : 16);      // WideTri
    w.bigRuns = take(p->leanMinClusters != 0u ? (uint64_t)p->leanQueue * 8 : 16);
    w.heldRecords = take(p->holdEnabled ? (uint64_t)c.maxVisibleClusters * sizeof(HeldRecord) : 16);
    w.lateList = take(p->holdEnabled ? (uint64_t)c.maxVisibleClusters * 4 : 16);
    w.wideQueue = take((uint64_t)std::max(1u, p->wideCapacity) * 96);      // WideTri (brmi_raster.hip)
    w.wideAlpha = take(p->tables.hasAlphaTest ? (uint64_t)std::max(1u, p->wideCapacity) * 48 : 16);
    w.shadowRecords = take((uint64_t)std::max(1u, p->scene.lightCount) * 32 + 32);              // the shading pass's 32 B shadow record per active light (brmi_shadow.h)
    w.total = off;
    p->resNeed[BRMI_RES_WORKSPACE] = w.total;
}

template <typename T>
static int read_back(brmi_pass* p, std::vector<T>& dst, const T* src, size_t n) {
    dst.resize(n);
    if (n == 0) return BRMI_OK;
    if (!src) return fail(p, BRMI_ERR_INVALID, "scene buffer missing");
    BRMI_HIP(p, hipMemcpy(dst.data(), src, n * sizeof(T), hipMemcpyDeviceToHost));
    return BRMI_OK;
}

}  // namespace brmi

brmi::HzbDesc brmi_pass::hzbDesc() const {
    brmi::HzbDesc d{};
    d.depth = static_cast<const float*>(res[BRMI_RES_LINEAR_DEPTH]); d.mips = static_cast<float*>(res[BRMI_RES_HZB]);
    d.width = cfg.width; d.height = cfg.height; d.tilesX = tilesX; d.mipCount = hzbMipCount; d.rowLo = bandY0; d.rowHi = bandY1; d.stripes = stripes;
    d.paddedW = hzbMipCount ? hzbMipW[0] : 1; d.paddedH = hzbMipCount ? hzbMipH[0] : 1;
    for (uint32_t i = 0; i < brmi::kMaxHzbMips; i++) d.mipOffset[i] = i < hzbMipCount ? (uint32_t)hzbMipOffsets[i] : 0u;
    return d;
}

using namespace brmi;

extern "C" {

uint32_t brmi_abi_version(void) { return BRMI_ABI_VERSION; }
uint32_t brmi_abi_minor(void) { return BRMI_ABI_MINOR; }

void brmi_default_config(brmi_config* cfg, uint32_t width, uint32_t height) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->structSize = sizeof(brmi_config);
    cfg->width = width; cfg->height = height;
    cfg->maxVisibleClusters = 1u << 22;       // reference: 30,000,000 (Renderer.cpp:2494); callers size it to the scene
    cfg->maxTraversalRecords = 1u << 22;
    cfg->enableOcclusionCulling = 0;          // opt-in: 2-phase HZB occlusion culling (needs a previous frame to pay off)
    cfg->enableClusteredLighting = 1;
    cfg->enablePunctualLights = 1;
    cfg->lightClusterSize[0] = 12; cfg->lightClusterSize[1] = 12; cfg->lightClusterSize[2] = 24;
    cfg->phase2ExpansionFactor = 2;
    cfg->collectPassStatistics = 0;
    cfg->maxBvhLevels = 64;
    cfg->keepUniformLayerPlanes = 0;          // opt-in: every plane is written every frame unless the host says the planes are its to keep
}

}  // extern "C"
namespace brmi {
// BRMI_TUNING="key=value,key=value": looked up on every call (a test sets it around the creation of one pass; nothing here is on a frame's path)
static bool tuning_lookup(const char* key, long* out) {
    const char* e = std::getenv("BRMI_TUNING");
    if (!e) return false;
    const size_t n = std::strlen(key);
    for (const char* q = e; *q; ) {
        while (*q == ',' || *q == ' ') q++;
        const char* end = std::strchr(q, ',');
        const size_t len = end ? (size_t)(end - q) : std::strlen(q);
        if (len > n && std::strncmp(q, key, n) == 0 && q[n] == '=') { *out = std::strtol(q + n + 1, nullptr, 0); return true; }
        q += len;
    }
    return false;
}
long tuning(const char* key, long def) { long v; return tuning_lookup(key, &v) ? v : def; }
}  // namespace brmi
extern "C" {

int brmi_create(const brmi_config* cfg, brmi_pass** out) {
    if (!cfg || !out || cfg->structSize != sizeof(brmi_config) || cfg->width == 0 || cfg->height == 0) return BRMI_ERR_INVALID;
    // (<= 2^25 - 1 clusters: the vertex and the triangle count sums of a frame's list share one 64-bit counter, 128 per cluster at most -- brmi_internal.h, CNT_SUM_VERTS_LO; the
    // reference's 30,000,000, Renderer.cpp:2494, fits)
    if (cfg->maxVisibleClusters == 0 || cfg->maxVisibleClusters > (1u << 25) - 1u || cfg->maxTraversalRecords == 0) return BRMI_ERR_INVALID;
    if (cfg->lightClusterSize[0] == 0 || cfg->lightClusterSize[1] == 0 || cfg->lightClusterSize[2] == 0) return BRMI_ERR_INVALID;
    if (cfg->lightClusterSize[2] > 62u) return BRMI_ERR_INVALID;
    if ((uint64_t)((cfg->width + 255u) / 256u) * ((cfg->height + 15u) / 16u) > 65535ull) return BRMI_ERR_INVALID;      // the raster bins' work items name a bin in 16 bits (16384 x 16368 px still fits)
    if (cfg->stripeCount > 1u) {      // interleaved partition: whole chunks of 16-row bin bands, the same number on every GPU, no band on top
        if (cfg->stripeRows == 0u || cfg->stripeRows % 16u || cfg->stripeIndex >= cfg->stripeCount || cfg->bandY0 != 0u || (cfg->bandY1 != 0u && cfg->bandY1 != cfg->height)) return BRMI_ERR_INVALID;
        if (cfg->fullHeight == 0u || cfg->fullHeight % (cfg->stripeRows * cfg->stripeCount) || cfg->height != cfg->fullHeight / cfg->stripeCount) return BRMI_ERR_INVALID;
        if (cfg->dynamicBand) return BRMI_ERR_INVALID;
    }
    if (cfg->dynamicBand && (cfg->bandY0 % 8u || (cfg->bandY1 % 8u && cfg->bandY1 < cfg->height))) return BRMI_ERR_INVALID;      // the slice-start table (workspace and the shading pass's LDS copy) holds 64 entries: gz + 2
    brmi_pass* p = new brmi_pass();
    p->cfg = *cfg;
    p->totalWords = 1; p->scanBlocks = 1;
    // sizes and switches a test (or a user) may set: BRMI_TUNING="key=value,..." 
    p->forceLevelKernels = tuning("cull_level_kernels", 0) != 0;
    p->packedFlat = tuning("flat_packed", 1) != 0;
    p->flatLevelsMinDraws = (uint32_t)std::max(0l, tuning("flat_levels_min_draws", p->flatLevelsMinDraws));      // (tests: 1 = the level-synchronous flat traversal for every scene)
    p->phase2DirectMax = (uint32_t)std::max(0l, tuning("phase2_direct_max", p->phase2DirectMax));
    p->resolveInlineMode = (int)tuning("resolve_inline", -1);
    p->wideCapacity = (uint32_t)std::min(1l << 20, std::max(0l, tuning("wide_capacity", p->wideCapacity)));
    p->wideMinTriangles = (uint32_t)std::max(0l, tuning("wide_min_triangles", p->wideMinTriangles));
    p->rasterSlim = (int)std::max(-1l, std::min(1l, tuning("raster_slim", -1)));      // 0 | 1: today's or the slim shape of k_raster on every frame; unset (or -1): launch_raster picks
    p->leanMinClusters = (uint32_t)std::max(0l, tuning("lean_min_clusters", p->leanMinClusters));
    if (p->leanMinClusters > cfg->maxVisibleClusters) p->leanMinClusters = 0u;      // a pass whose list cannot get that long never runs the lean rasteriser: no queue in its workspace (104 MB)
    p->leanMaxGeneralPct = (uint32_t)std::max(0l, std::min(100l, tuning("lean_max_general_pct", p->leanMaxGeneralPct)));
    p->leanGrid = (uint32_t)std::max(64l, tuning("lean_grid", p->leanGrid));
    p->leanQueue = (uint32_t)std::max(64l, std::min(1l << 24, tuning("lean_queue", p->leanQueue))) & ~63u;      // (64 stripes)
    p->leanWideEntries = (uint32_t)std::max(1l, tuning("lean_wide_entries", p->leanWideEntries));
    p->leanEmitGrid = (uint32_t)std::max(64l, std::min(65536l, tuning("lean_emit_grid", p->leanEmitGrid))) & ~63u;
    p->wideEntries = (uint32_t)std::max(1l, tuning("wide_entries", p->wideEntries));
    p->binMinSlice = (uint32_t)std::max(32l, tuning("bin_min_slice", p->binMinSlice));
    p->binSharedSlice = (uint32_t)std::max(32l, tuning("bin_shared_slice", p->binSharedSlice));
    p->binGrid = (uint32_t)std::min(65535l, std::max(1l, tuning("bin_grid", p->binGrid)));
    p->binOverflowPerStripe = (uint32_t)std::max(0l, tuning("bin_overflow", p->binOverflowPerStripe));
    p->binCapacity = (uint32_t)std::min(65536l, std::max(1l, tuning("bin_capacity", p->binCapacity)));   // 16-bit record indices inside a bin slice's alpha list; 65536 x 64 B x bins is far beyond any frame
    if (const long v = tuning("big_tri_area", 0)) p->bigTriArea = p->bigTriAreaAlpha = p->bigTriAreaDense = (int)std::max(1l, v);
    compute_sizes(p);
    *out = p;
    return BRMI_OK;
}

void brmi_destroy(brmi_pass* p) {
    if (!p) return;
    if (p->eventsCreated) for (int i = 0; i < BRMI_STAGE_COUNT; i++) for (uint32_t k = 0; k < brmi_pass::kEventRing; k++) { (void)hipEventDestroy(p->evStart[i][k]); (void)hipEventDestroy(p->evStop[i][k]); }
    (void)brmi_set_history_source(p, nullptr);
    for (brmi_pass* user : p->historyUsers) user->history = nullptr;
    if (p->chainReady) (void)hipEventDestroy(p->chainReady);
    if (p->geometryDone) (void)hipEventDestroy(p->geometryDone);
    if (p->cullDone) (void)hipEventDestroy(p->cullDone);
    if (p->frameDone) (void)hipEventDestroy(p->frameDone);
    p->feedback.release();
    delete p;
}

// the stages that need no pass (brmi_texmips_*) leave their refusal here, per calling thread; brmi_last_error(NULL) reads it
static thread_local std::string g_stageError;
static int stage_fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); brmi::vrefuse(g_stageError, code, fmt, ap); va_end(ap);
    return code;
}
const char* brmi_last_error(const brmi_pass* p) { return p ? p->err.c_str() : (g_stageError.empty() ? "null pass" : g_stageError.c_str()); }

// Provider resolution.  Copies the scene's arrays to the host once and hands them to analyse_scene (brmi_scene_tables.h), which
// validates the cross references and derives brmi_pass::tables; what follows sizes the workspace from them.
int brmi_set_scene(brmi_pass* p, const brmi_scene_buffers* scene) {
    if (!p || !scene) return BRMI_ERR_INVALID;
    p->scene = *scene; p->haveScene = false; p->setupDone = false;
    p->streaming.on = false;      // (bound to the group table of the scene before: brmi_set_streaming again)
    p->samplerAniso = nullptr;    // (one word per sampler of the scene before: brmi_set_sampler_anisotropy again)
    p->temporal.valid = false;    // (last frame's resolved image shows another scene: the next resolve writes the current frame)
    p->shadows.on = false; p->shadows.b = brmi_shadow_buffers{};      // (validated against the lights and cameras of the scene before: brmi_set_shadows again)
    const brmi_scene_buffers& sc = p->scene;
    if (!sc.slabs || !sc.perObject || !sc.perMesh || !sc.perMeshInstance || !sc.clodOffsets || !sc.meshMetadata || !sc.lodNodes || !sc.lodGroups ||
        !sc.lodSegments || !sc.groupPageMap || !sc.materials || !sc.openpbrMaterials || !sc.cameras || !sc.cullingCameras || !sc.viewRasterInfo || !sc.perFrame ||
        !sc.normalMatrices || (sc.activeDrawCount && !sc.activeDraws) || (sc.lightCount && (!sc.lights || !sc.activeLightIndices)))
        return fail(p, BRMI_ERR_INVALID, "brmi_set_scene: a required scene buffer is null");
    if (!sc.lutOpaqueDielectricEnergyComplement || !sc.lutOpaqueDielectricAvgEnergyComplement || !sc.lutIdealMetalEnergyComplement || !sc.lutIdealMetalAvgEnergyComplement || !sc.lutFuzzLTC)
        return fail(p, BRMI_ERR_INVALID, "brmi_set_scene: OpenPBR lookup tables must be provided");
    // every array the analysis reads, copied to the host once (brmi_scene_tables.h: HostScene)
    HostScene hs; int rc;
    if ((rc = read_back(p, hs.meshMetadata, sc.meshMetadata, sc.meshMetadataCount))) return rc;
    if ((rc = read_back(p, hs.clodOffsets, sc.clodOffsets, sc.perMeshInstanceCount))) return rc;
    if ((rc = read_back(p, hs.lodNodes, sc.lodNodes, sc.lodNodeCount))) return rc;
    if ((rc = read_back(p, hs.lodSegments, sc.lodSegments, sc.lodSegmentCount))) return rc;
    if ((rc = read_back(p, hs.openpbrMaterials, sc.openpbrMaterials, sc.openpbrMaterialCount))) return rc;
    if ((rc = read_back(p, hs.materials, sc.materials, sc.materialCount))) return rc;
    if ((rc = read_back(p, hs.perMesh, sc.perMesh, sc.perMeshCount))) return rc;
    if ((rc = read_back(p, hs.perMeshInstance, sc.perMeshInstance, sc.perMeshInstanceCount))) return rc;
    if ((rc = read_back(p, hs.activeDraws, sc.activeDraws, sc.activeDrawCount))) return rc;
    if ((rc = read_back(p, hs.groupPageMap, sc.groupPageMap, sc.groupPageMapCount))) return rc;
    if ((rc = read_back(p, hs.lodGroups, sc.lodGroups, sc.lodGroupCount))) return rc;
    if ((rc = read_back(p, hs.slabs, sc.slabs, sc.slabCount))) return rc;
    hs.perObjectCount = sc.perObjectCount; hs.skinningMatrixCount = sc.skinningMatrixCount;      // (nothing reads the contents of perObject or of the matrices)
    hs.textureTables = sc.textures && sc.samplers && sc.srgbToLinear && sc.textureCount != 0 && sc.samplerCount != 0;
    const bool flatOn = tuning("flat_traversal", 1) != 0;
    const bool boxesOn = tuning("hold_clusters", 1) != 0 && p->cfg.enableOcclusionCulling && sc.slabCount <= 4096u;
    const auto pageMeshlets = [&](uint32_t slab, uint32_t byteOffset, uint32_t* meshlets) -> int { BRMI_HIP(p, hipMemcpy(meshlets, hs.slabs[slab] + byteOffset, 4, hipMemcpyDeviceToHost)); return BRMI_OK; };
    if ((rc = analyse_scene(hs, flatOn, p->cfg.maxBvhLevels, boxesOn, pageMeshlets, p->tables, p->err))) return rc;
    // (the interleaved partition keeps the whole list: its compact surfaces hold this GPU's chunks only -- the re-test would have to map rows.  A contiguous band
    // lives in frame rows: the tests clamp their rectangles to it, and the chain's texels beyond it read "empty")
    p->holdEnabled = boxesOn && p->tables.totalBoxes != 0u && p->stripes.count <= 1u;
    p->holdMinClusters = (uint32_t)std::max(0l, tuning("hold_min_clusters", p->holdMinClusters));
    p->lateDirectMax = (uint32_t)std::max(0l, tuning("late_direct_max", p->lateDirectMax));
    p->holdStillMax = (uint32_t)std::max(0l, tuning("hold_still_max", p->holdStillMax));
    p->holdFloor = (uint32_t)std::max(0l, tuning("hold_floor", p->holdFloor));
    p->holdMaxTexels = (uint32_t)std::min(16l, std::max(1l, tuning("hold_max_texels", p->holdMaxTexels)));
    p->retestMaxTexels = (uint32_t)std::min(16l, std::max(1l, tuning("retest_max_texels", p->retestMaxTexels)));
    p->totalWords = (uint32_t)std::max<uint64_t>(1, (p->tables.totalBits + 31) / 32);
    p->scanBlocks = (p->totalWords + 2047u) / 2048u;
    p->maxLevels = std::min(std::max(1u, p->tables.maxDepth), std::max(1u, p->cfg.maxBvhLevels));
    compute_sizes(p);
    p->haveScene = true;
    p->updateSerial++;
    return BRMI_OK;
}

int brmi_set_band(brmi_pass* p, uint32_t bandY0, uint32_t bandY1) {
    if (!p) return BRMI_ERR_INVALID;
    if (!p->cfg.dynamicBand) return fail(p, BRMI_ERR_STATE, "brmi_set_band: the pass was created without brmi_config::dynamicBand");
    if (bandY1 > p->cfg.height) bandY1 = p->cfg.height;
    if (bandY0 % 8u || (bandY1 % 8u && bandY1 != p->cfg.height) || bandY0 >= bandY1) return fail(p, BRMI_ERR_INVALID, "brmi_set_band: rows [%u, %u) -- multiples of 8 inside the frame's %u rows", bandY0, bandY1, p->cfg.height);
    p->bandY0 = bandY0; p->bandY1 = bandY1;
    const uint32_t t0 = bandY0 / 8u, t1 = (bandY1 + 7u) / 8u;
    p->bandFirstPixel = (uint64_t)t0 * p->tilesX * 64; p->bandPixelCount = (uint64_t)(t1 - t0) * p->tilesX * 64;
    p->updated = false;      // the band planes of the culling are made by brmi_update
    return BRMI_OK;
}

int brmi_declare(brmi_pass* p, brmi_declare_cb cb, void* user) {
    if (!p || !cb) return BRMI_ERR_INVALID;
    if (!p->haveScene) return fail(p, BRMI_ERR_STATE, "brmi_declare: call brmi_set_scene first (workspace size depends on the scene)");
    for (uint32_t i = 0; i < BRMI_RES_COUNT; i++) {
        brmi_resource_desc d{};
        d.id = i; d.name = kResNames[i]; d.bytes = p->resNeed[i];
        const bool image = i <= BRMI_RES_HDR_COLOR;
        d.usage = BRMI_USAGE_UNORDERED_ACCESS | BRMI_USAGE_SHADER_RESOURCE | ((i == BRMI_RES_WORKSPACE || i == BRMI_RES_HZB) ? BRMI_USAGE_INTERNAL : 0u);
        d.width = image ? p->cfg.width : 0; d.height = image ? p->cfg.height : 0; d.bytesPerPixel = kResBpp[i];
        d.tileW = image ? 8 : 0; d.tileH = image ? 8 : 0;
        cb(user, &d);
    }
    return BRMI_OK;
}

int brmi_setup(brmi_pass* p, const brmi_resource_binding* b, uint32_t n, brmi_stream stream) {
    if (!p || (!b && n)) return BRMI_ERR_INVALID;
    if (!p->haveScene) return fail(p, BRMI_ERR_STATE, "brmi_setup: call brmi_set_scene first");
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (uint32_t i = 0; i < n; i++) {
        if (b[i].id >= BRMI_RES_COUNT) return fail(p, BRMI_ERR_INVALID, "brmi_setup: unknown resource id %u", b[i].id);
        p->res[b[i].id] = b[i].ptr; p->resBytes[b[i].id] = b[i].bytes;
    }
    for (uint32_t i = 0; i < BRMI_RES_COUNT; i++) {
        if (!p->res[i]) return fail(p, BRMI_ERR_INVALID, "brmi_setup: resource %s not bound", kResNames[i]);
        if (p->resBytes[i] < p->resNeed[i]) return fail(p, BRMI_ERR_CAPACITY, "brmi_setup: resource %s is %llu B, needs %llu B", kResNames[i], (unsigned long long)p->resBytes[i], (unsigned long long)p->resNeed[i]);
        if ((reinterpret_cast<uintptr_t>(p->res[i]) & 15u) != 0) return fail(p, BRMI_ERR_INVALID, "brmi_setup: resource %s must be 16-byte aligned", kResNames[i]);
    }
    BRMI_HIP(p, hipMemsetAsync(p->res[BRMI_RES_WORKSPACE], 0, p->ws.total, s));
    // the depth chain starts out "empty" everywhere; a multi-GPU band only ever rewrites the texels its rows reach
    if (p->cfg.enableOcclusionCulling && p->resNeed[BRMI_RES_HZB] >= 4) BRMI_HIP(p, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p->res[BRMI_RES_HZB]), (int)BRMI_DEPTH_EMPTY_BITS, p->resNeed[BRMI_RES_HZB] / 4, s));
    p->hzbValid = false;
    if (!p->tables.instanceBitBase.empty()) BRMI_HIP(p, hipMemcpyAsync(p->wsPtr<uint32_t>(p->ws.instanceBitBase), p->tables.instanceBitBase.data(), p->tables.instanceBitBase.size() * 4, hipMemcpyHostToDevice, s));
    if (!p->tables.segPrefix.empty()) BRMI_HIP(p, hipMemcpyAsync(p->wsPtr<uint32_t>(p->ws.segPrefix), p->tables.segPrefix.data(), p->tables.segPrefix.size() * 4, hipMemcpyHostToDevice, s));
    if (!p->tables.meshLevelWidth.empty()) BRMI_HIP(p, hipMemcpyAsync(p->wsPtr<uint32_t>(p->ws.meshLevelWidth), p->tables.meshLevelWidth.data(), p->tables.meshLevelWidth.size() * 4, hipMemcpyHostToDevice, s));
    if (!p->tables.flatNodes.empty()) BRMI_HIP(p, hipMemcpyAsync(p->wsPtr<FlatNode>(p->ws.flatNodes), p->tables.flatNodes.data(), p->tables.flatNodes.size() * sizeof(FlatNode), hipMemcpyHostToDevice, s));
    if (!p->tables.flatLeaves.empty()) BRMI_HIP(p, hipMemcpyAsync(p->wsPtr<FlatLeaf>(p->ws.flatLeaves), p->tables.flatLeaves.data(), p->tables.flatLeaves.size() * sizeof(FlatLeaf), hipMemcpyHostToDevice, s));
    if (!p->tables.instanceWalk.empty()) BRMI_HIP(p, hipMemcpyAsync(p->wsPtr<InstanceWalk>(p->ws.instanceWalk), p->tables.instanceWalk.data(), p->tables.instanceWalk.size() * sizeof(InstanceWalk), hipMemcpyHostToDevice, s));
    if (!p->tables.pageBoxBase.empty()) BRMI_HIP(p, hipMemcpyAsync(p->wsPtr<uint32_t>(p->ws.pageBoxBase), p->tables.pageBoxBase.data(), p->tables.pageBoxBase.size() * 4, hipMemcpyHostToDevice, s));
    if (!p->tables.pageRefs.empty()) BRMI_HIP(p, hipMemcpyAsync(p->wsPtr<PageRef>(p->ws.pageRefs), p->tables.pageRefs.data(), p->tables.pageRefs.size() * sizeof(PageRef), hipMemcpyHostToDevice, s));
    { int rc = launch_expand_luts(p, s); if (rc) return rc; }
    { int rc = launch_meshlet_boxes(p, s); if (rc) return rc; }
    BRMI_HIP(p, hipStreamSynchronize(s));   // host vectors may be reused
    if (p->cfg.collectPassStatistics && !p->eventsCreated) {
        for (int i = 0; i < BRMI_STAGE_COUNT; i++) for (uint32_t k = 0; k < brmi_pass::kEventRing; k++) { BRMI_HIP(p, hipEventCreate(&p->evStart[i][k])); BRMI_HIP(p, hipEventCreate(&p->evStop[i][k])); }
        p->eventsCreated = true;
    }
    p->setupDone = true;
    p->layerPlanesDirty = true;      // new (or re-bound) G-buffer planes: the uniform coat / fuzz words have to be filled in again
    p->constantsSerial = 0;      // the workspace was cleared: the frame constants have to be evaluated again
    return BRMI_OK;
}

// Per-frame host work.  The slice plane depths of the light-cluster grid are evaluated here with
// logf/expf (clustering.hlsl:66-90 evaluates them per cluster on the GPU).
int brmi_update(brmi_pass* p, const brmi_frame_update* u, brmi_stream stream) {
    if (!p || !u || !u->mainCameraHost || !u->perFrameHost) return BRMI_ERR_INVALID;
    if (!p->setupDone) return fail(p, BRMI_ERR_STATE, "brmi_update: call brmi_setup first");
    if (p->env.on && u->perFrameHost->activeEnvironmentIndex >= p->env.b.environmentCount)      // (before anything of the pass changes: the frame before stays the last one)
        return fail(p, BRMI_ERR_INVALID, "brmi_update: perFrame.activeEnvironmentIndex %u, the bound environment table has %u entries", u->perFrameHost->activeEnvironmentIndex, p->env.b.environmentCount);
    p->camHost = *u->mainCameraHost; p->pfHost = *u->perFrameHost; p->frameIndexHost = u->frameIndex;
    const brmi_per_frame& pf = p->pfHost;
    if (pf.lightClusterGridSizeX != p->cfg.lightClusterSize[0] || pf.lightClusterGridSizeY != p->cfg.lightClusterSize[1] || pf.lightClusterGridSizeZ != p->cfg.lightClusterSize[2])
        return fail(p, BRMI_ERR_INVALID, "brmi_update: per-frame light cluster grid differs from the configured lightClusterSize");
    if (pf.screenResX != p->cfg.width || pf.screenResY != p->frameHeight()) return fail(p, BRMI_ERR_INVALID, "brmi_update: per-frame screen size differs from the configured target size");
    const float zNear = p->camHost.zNear, zFar = p->camHost.zFar, zSplit = pf.clusterZSplitDepth;
    const uint32_t gz = pf.lightClusterGridSizeZ, nearSlices = pf.nearClusterCount;
    p->planesHost.resize(2 * gz);
    for (uint32_t sliceZ = 0; sliceZ < gz; sliceZ++) {
        float pn, pfar;
        if (sliceZ < nearSlices) {
            const float sliceSize = (zSplit - zNear) / (float)nearSlices;
            pn = -(zNear + (float)sliceZ * sliceSize);
            pfar = -(zNear + (float)(sliceZ + 1) * sliceSize);
        } else {
            const float logStart = std::log(zSplit / zNear), logEnd = std::log(zFar / zNear);
            const float t0 = (float)(sliceZ - nearSlices) / (float)(gz - nearSlices);
            const float t1 = (float)(sliceZ + 1 - nearSlices) / (float)(gz - nearSlices);
            pn = -zNear * std::exp(logStart + t0 * (logEnd - logStart));
            pfar = -zNear * std::exp(logStart + t1 * (logEnd - logStart));
        }
        p->planesHost[2 * sliceZ] = pn; p->planesHost[2 * sliceZ + 1] = pfar;
    }
    // sliceStart[s] = smallest view depth whose cluster slice (ComputeClusterID, lighting.hlsli:166-196) is >= s: the formula is monotone in
    // depth, so the shading pass finds a pixel's slice by comparing against this table instead of two divisions and a logarithm.  Bisection
    // over the positive floats with the shader's own formula; `log` is the correctly rounded fp32 logarithm (through fp64).  Re-evaluated
    // only when the depth range or the grid changes.
    if (p->sliceStartHost.empty() || p->sliceKey[0] != zNear || p->sliceKey[1] != zFar || p->sliceKey[2] != zSplit || p->sliceKeyN[0] != nearSlices || p->sliceKeyN[1] != gz) {
        auto log_cr = [](float x) { return (float)std::log((double)x); };
        const float logStart = log_cr(zSplit / zNear), logEnd = log_cr(zFar / zNear);
        auto slice_of = [&](float z) -> uint32_t {
            if (z < zSplit) { const float t = (z - zNear) / (zSplit - zNear); return t > 0.0f ? (uint32_t)std::min(t * (float)nearSlices, 4294967040.0f) : 0u; }
            const float logZ = log_cr(z / zNear);
            const float u = (logZ - logStart) / (logEnd - logStart);
            return nearSlices + (u > 0.0f ? (uint32_t)std::min(u * (float)(gz - nearSlices), 4294967040.0f) : 0u);
        };
        auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
        auto flt = [](uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; };
        p->sliceStartHost.assign(gz + 2, 0.0f);
        p->sliceStartHost[gz + 1] = flt(0x7F800000u);
        for (uint32_t i = 1; i <= gz; i++) {
            // lo fails, hi passes.  The search stops at 1e30 (z / zNear must stay finite for the float -> uint conversion of the formula to
            // be defined); a slice that starts beyond it starts at +inf.
            uint32_t lo = 0u, hi = bits(1.0e30f);
            if (slice_of(1.0e30f) < i) lo = hi = 0x7F800000u;
            while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (slice_of(flt(mid)) >= i) hi = mid; else lo = mid; }
            p->sliceStartHost[i] = flt(hi);
        }
        p->sliceKey[0] = zNear; p->sliceKey[1] = zFar; p->sliceKey[2] = zSplit; p->sliceKeyN[0] = nearSlices; p->sliceKeyN[1] = gz;
    }
    {   // band planes of the screen-tile split, 2 px of slack (view space, through the eye)
        const float projY = p->camHost.projection[1][1], H = (float)p->frameHeight();
        const float T = 1.0f - 2.0f * ((float)p->bandY0 - 2.0f) / H, B = 1.0f - 2.0f * ((float)p->bandY1 + 2.0f) / H;
        const float lt = std::sqrt(projY * projY + T * T), lb = std::sqrt(projY * projY + B * B);
        p->bandPlaneTop[0] = 0.0f; p->bandPlaneTop[1] = -projY / lt; p->bandPlaneTop[2] = -T / lt;
        p->bandPlaneBottom[0] = 0.0f; p->bandPlaneBottom[1] = projY / lb; p->bandPlaneBottom[2] = B / lb;
    }
    (void)stream;      // nothing is uploaded: the slice planes are kernel arguments of the light clustering, everything else is derived on the device
    p->updated = true;
    p->updateSerial++;       // the per-frame constants are re-evaluated by the next stage call
    return BRMI_OK;
}

#define STAGE_BEGIN(p, st, s) do { if ((p)->eventsCreated && (((p)->timedStages >> (st)) & 1u)) { (void)hipEventRecord((p)->evStart[st][(p)->evCount[st] % brmi_pass::kEventRing], (s)); } } while (0)
#define STAGE_END(p, st, s) do { if ((p)->eventsCreated && (((p)->timedStages >> (st)) & 1u)) { (void)hipEventRecord((p)->evStop[st][(p)->evCount[st] % brmi_pass::kEventRing], (s)); (p)->evCount[st]++; } } while (0)
#define CHECK_READY(p) do { if (!(p)) return BRMI_ERR_INVALID; if (!(p)->setupDone || !(p)->updated) return brmi::fail((p), BRMI_ERR_STATE, "%s: setup/update not done", __func__); } while (0)

// What a frame's first launch has to wait for when frames are in flight (brmi_execute_split, and the stage entry points that start a frame:
// a graph that schedules the stages itself after a split frame gets the same ordering).  No-ops when nothing was recorded.
static int wait_for_frames_in_flight(brmi_pass* p, brmi_stream stream) {
    // this pass's previous frame may still be resolving / shading on the other stream: its visibility buffer and tables are about to be rewritten
    if (p->frameDoneRecorded) BRMI_HIP(p, hipStreamWaitEvent(static_cast<hipStream_t>(stream), p->frameDone, 0));
    p->frameDoneRecorded = false;
    // frames in flight: this frame's phase 1 reads the chain the source pass built for the frame before, possibly on another stream
    // (recorded on this very stream -- the passes of a ring share their geometry stream --: stream order already says so, and every wait
    // is a barrier packet worth a few us on the geometry half's critical path)
    if (p->history && p->history->chainRecorded && p->history->chainStream != stream) BRMI_HIP(p, hipStreamWaitEvent(static_cast<hipStream_t>(stream), p->history->chainReady, 0));
    // ... and this frame rewrites the chain a pass that has THIS one as its source may still be reading in its phase 1 (the same event:
    // it is recorded after that pass's culling)
    for (brmi_pass* user : p->historyUsers) if (user != p->history && user->chainRecorded && user->chainStream != stream) BRMI_HIP(p, hipStreamWaitEvent(static_cast<hipStream_t>(stream), user->chainReady, 0));
    return BRMI_OK;
}

// The stage bodies: a launcher between its stage's two timing events, with the frame's context -- brmi_execute_split's own, or the default one of a public entry point
// (readiness check, the in-flight waits where the stage can start a frame): a stage on its own takes no shortcut and leaves none behind.
static int stage_clear(brmi_pass* p, brmi::FrameCtx& ctx, brmi_stream stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    STAGE_BEGIN(p, BRMI_STAGE_CLEAR, s); int rc = launch_clear(p, ctx, s); STAGE_END(p, BRMI_STAGE_CLEAR, s); return rc;
}
static int stage_cull(brmi_pass* p, brmi::FrameCtx& ctx, uint32_t phase, brmi_stream stream) {
    hipStream_t s = static_cast<hipStream_t>(stream); const int st = phase == 2 ? BRMI_STAGE_CULL2 : BRMI_STAGE_CULL;
    STAGE_BEGIN(p, st, s); int rc = launch_cull(p, ctx, phase, s); STAGE_END(p, st, s); return rc;
}
static int stage_raster(brmi_pass* p, brmi::FrameCtx& ctx, uint32_t phase, brmi_stream stream) {
    hipStream_t s = static_cast<hipStream_t>(stream); const int st = phase == 2 ? BRMI_STAGE_RASTER2 : BRMI_STAGE_RASTER;
    STAGE_BEGIN(p, st, s); int rc = launch_raster(p, ctx, phase, s); STAGE_END(p, st, s); return rc;
}
// brmi_execute's chain builds: (1) LinearDepthCopyPass1 + LinearDepthDownsamplePass1 in one kernel (the chain is built straight from the visibility keys, the depth map is
// written on the way); (2) LinearDepthDownsamplePass2 skipped on the device when phase 2 rasterised nothing, because the final depth then equals the phase-1 depth
static int stage_hzb(brmi_pass* p, brmi::FrameCtx& ctx, brmi_stream stream, brmi::ChainBuild build) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    STAGE_BEGIN(p, BRMI_STAGE_HZB, s); int rc = launch_hzb(p, ctx, s, build); STAGE_END(p, BRMI_STAGE_HZB, s);
    if (rc == BRMI_OK) p->hzbValid = true;
    return rc;
}
static int stage_gbuffer(brmi_pass* p, brmi::FrameCtx& ctx, brmi_stream stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    STAGE_BEGIN(p, BRMI_STAGE_GBUFFER, s); int rc = launch_gbuffer(p, ctx, s); STAGE_END(p, BRMI_STAGE_GBUFFER, s); return rc;
}
static int stage_light_clustering(brmi_pass* p, brmi::FrameCtx& ctx, brmi_stream stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    STAGE_BEGIN(p, BRMI_STAGE_LIGHT_CLUSTER, s); int rc = launch_light_clustering(p, ctx, s); STAGE_END(p, BRMI_STAGE_LIGHT_CLUSTER, s); return rc;
}
static int stage_shade(brmi_pass* p, brmi::FrameCtx& ctx, brmi_stream stream, bool withGtao = false) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    STAGE_BEGIN(p, BRMI_STAGE_SHADE, s);
    int rc = BRMI_OK;
    if (withGtao) { rc = launch_gtao_prefilter(p, s); if (!rc) rc = launch_gtao_main(p, s); if (!rc) rc = launch_gtao_denoise(p, s); }
    if (!rc) rc = launch_shade(p, ctx, s);
    STAGE_END(p, BRMI_STAGE_SHADE, s); return rc;
}

int brmi_clear_visibility(brmi_pass* p, brmi_stream stream) {
    CHECK_READY(p); brmi::FrameCtx ctx;
    if (int w = wait_for_frames_in_flight(p, stream)) return w;
    return stage_clear(p, ctx, stream);
}
int brmi_cull(brmi_pass* p, uint32_t phase, brmi_stream stream) {
    CHECK_READY(p); brmi::FrameCtx ctx;
    if (phase == 1) if (int w = wait_for_frames_in_flight(p, stream)) return w;
    return stage_cull(p, ctx, phase, stream);
}
int brmi_raster(brmi_pass* p, uint32_t phase, brmi_stream stream) { CHECK_READY(p); brmi::FrameCtx ctx; return stage_raster(p, ctx, phase, stream); }
int brmi_depth_copy(brmi_pass* p, brmi_stream stream) {
    CHECK_READY(p); hipStream_t s = static_cast<hipStream_t>(stream);
    STAGE_BEGIN(p, BRMI_STAGE_DEPTH_COPY, s); int rc = launch_depth_copy(p, s); STAGE_END(p, BRMI_STAGE_DEPTH_COPY, s); return rc;
}
uint64_t brmi_streaming_scratch_bytes(uint32_t lodGroupCount) { return brmi::stream_scratch_layout(lodGroupCount).total; }
int brmi_set_streaming(brmi_pass* p, const brmi_streaming_buffers* b) {
    if (!p) return BRMI_ERR_INVALID;
    if (!b) { p->streaming.on = false; return BRMI_OK; }
    if (!p->haveScene) return brmi::fail(p, BRMI_ERR_STATE, "brmi_set_streaming: brmi_set_scene first (the buffers are sized by its group table)");
    if (b->structSize != sizeof(brmi_streaming_buffers)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_streaming: structSize %u, expected %zu", b->structSize, sizeof(brmi_streaming_buffers));
    if (!b->nonResidentBits || !b->counts || !b->scratch || (b->requestCapacity && !b->loadRequests) || (b->touchedCapacity && !b->touchedGroups))
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_streaming: a required streaming buffer is null");
    const uint64_t need = brmi_streaming_scratch_bytes(p->scene.lodGroupCount);
    if (b->scratchBytes < need) return brmi::fail(p, BRMI_ERR_CAPACITY, "brmi_set_streaming: scratch holds %llu bytes, %u groups need %llu", (unsigned long long)b->scratchBytes, p->scene.lodGroupCount, (unsigned long long)need);
    if (reinterpret_cast<uintptr_t>(b->scratch) & 15u) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_streaming: scratch must be 16 B aligned");
    p->streaming.b = *b; p->streaming.groupCount = p->scene.lodGroupCount;
    p->streaming.activeGroupScanCount = std::min(b->activeGroupScanCount, p->scene.lodGroupCount);
    p->streaming.on = true;
    return BRMI_OK;
}
int brmi_set_sampler_anisotropy(brmi_pass* p, const uint32_t* maxAnisotropy, uint32_t count) {
    if (!p) return BRMI_ERR_INVALID;
    if (!maxAnisotropy) { p->samplerAniso = nullptr; return BRMI_OK; }
    if (!p->haveScene) return brmi::fail(p, BRMI_ERR_STATE, "brmi_set_sampler_anisotropy: brmi_set_scene first (the table has one word per sampler of the scene)");
    if (count != p->scene.samplerCount) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_sampler_anisotropy: count %u, the scene has %u samplers", count, p->scene.samplerCount);
    p->samplerAniso = maxAnisotropy;
    return BRMI_OK;
}
// brmi_environment_buffers grew by `skybox`: the struct of either size is taken, the field is read only where structSize covers it
static bool environment_struct_size_ok(uint32_t structSize) { return structSize == sizeof(brmi_environment_buffers) || structSize == BRMI_ENVIRONMENT_BUFFERS_SIZE_V1; }
// the caller's struct of either size as the grown one: the first layout's fields, then `skybox` where structSize covers it (nothing past the caller's object is read)
static brmi_environment_buffers environment_struct_of(const brmi_environment_buffers* e) {
    brmi_environment_buffers b{};
    b.structSize = (uint32_t)sizeof(b); b.specularIBL = e->specularIBL; b.environments = e->environments; b.environmentCount = e->environmentCount;
    b.cubemaps = e->cubemaps; b.cubemapCount = e->cubemapCount;
    b.skybox = e->structSize >= offsetof(brmi_environment_buffers, skybox) + sizeof(uint32_t) && e->skybox != 0u ? 1u : 0u;
    return b;
}
int brmi_set_environment(brmi_pass* p, const brmi_environment_buffers* e) {
    if (!p) return BRMI_ERR_INVALID;
    if (!e) { if (p->env.on) p->updateSerial++; p->env.on = false; p->env.b = brmi_environment_buffers{}; return BRMI_OK; }
    if (!environment_struct_size_ok(e->structSize))
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_environment: structSize %u, expected %zu (or %u, the struct before `skybox`)", e->structSize, sizeof(brmi_environment_buffers), BRMI_ENVIRONMENT_BUFFERS_SIZE_V1);
    if ((!e->environments && e->environmentCount) || (!e->cubemaps && e->cubemapCount)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_environment: a null table with a non-zero count");
    if (e->environmentCount == 0u || !e->environments) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_environment: environmentCount is 0 (NULL unbinds)");
    if (p->updated && p->pfHost.activeEnvironmentIndex >= e->environmentCount)
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_environment: the last brmi_update's activeEnvironmentIndex is %u, the table has %u entries", p->pfHost.activeEnvironmentIndex, e->environmentCount);
    p->env.b = environment_struct_of(e); p->env.on = true;
    p->updateSerial++;       // the frame constants fold the environment's coefficients: re-evaluated by the next stage call
    return BRMI_OK;
}
// what keeps the skybox stage from running, checked by the stage and by brmi_execute_split in front of a frame's first launch (as debug_view_refusal is)
static int skybox_refusal(brmi_pass* p) {
    if (!p->setupDone) return brmi::fail(p, BRMI_ERR_STATE, "brmi_skybox: call brmi_setup first");
    if (!p->updated) return brmi::fail(p, BRMI_ERR_STATE, "brmi_skybox: call brmi_update first (the environment is perFrame.activeEnvironmentIndex of the last update)");
    if (!p->env.on || !p->env.b.skybox) return brmi::fail(p, BRMI_ERR_STATE, "brmi_skybox: no environment with `skybox` set is bound (brmi_set_environment)");
    if (!p->res[BRMI_RES_LINEAR_DEPTH] || !p->res[BRMI_RES_HDR_COLOR] || !p->res[BRMI_RES_GBUF_MOTION_VECTORS]) return brmi::fail(p, BRMI_ERR_STATE, "brmi_skybox: the depth, HDR or motion-vector surface is not bound");
    return BRMI_OK;
}
int brmi_skybox(brmi_pass* p, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (int rc = skybox_refusal(p)) return rc;
    return brmi::launch_skybox(p, static_cast<hipStream_t>(stream));
}

// ---- environment build (brmi_envbuild.hip): every refusal comes before the first launch
static bool env_size_ok(uint32_t size) { return size != 0u && size <= 16384u; }
int brmi_env_convert(const brmi_texture_desc* equirect, const brmi_texture_desc* cube, uint32_t size, uint32_t cubeFormat, brmi_stream stream) {
    if (!equirect || !cube || !env_size_ok(size) || cubeFormat != BRMI_TEXTURE_FORMAT_RGBA16_FLOAT) return BRMI_ERR_INVALID;
    return brmi::launch_env_convert(equirect, cube, size, static_cast<hipStream_t>(stream));
}
int brmi_env_project_sh(const brmi_texture_desc* cubemaps, uint32_t cubemapCount, brmi_environment_info* environments, uint32_t environmentCount, uint32_t environmentIndex, uint32_t size, brmi_stream stream) {
    if (!cubemaps || cubemapCount == 0u || !environments || environmentIndex >= environmentCount || !env_size_ok(size)) return BRMI_ERR_INVALID;
    return brmi::launch_env_project_sh(cubemaps, cubemapCount, environments + environmentIndex, size, static_cast<hipStream_t>(stream));
}
int brmi_env_prefilter(const brmi_texture_desc* sourceCube, const brmi_texture_desc* prefiltered, uint32_t size, uint32_t levels, uint32_t prefilteredFormat, brmi_stream stream) {
    if (!sourceCube || !prefiltered || !env_size_ok(size) || levels == 0u || levels > BRMI_TEXTURE_MAX_MIPS || prefilteredFormat != BRMI_TEXTURE_FORMAT_RGBA8_UNORM) return BRMI_ERR_INVALID;
    return brmi::launch_env_prefilter(sourceCube, prefiltered, size, levels, static_cast<hipStream_t>(stream));
}
uint64_t brmi_env_build_bytes(uint32_t size, uint32_t levels, uint64_t* cubeBytes, uint64_t* prefilteredBytes) {
    if (cubeBytes) *cubeBytes = 0; if (prefilteredBytes) *prefilteredBytes = 0;
    if (!env_size_ok(size) || levels == 0u || levels > BRMI_TEXTURE_MAX_MIPS) return 0;
    const uint64_t cube = 6ull * size * size * 8ull;
    uint64_t chain = 0;
    for (uint32_t m = 0; m < levels; m++) { const uint64_t s = std::max(1u, size >> m); chain += s * s; }
    chain *= 6ull * 4ull;
    if (cubeBytes) *cubeBytes = cube; if (prefilteredBytes) *prefilteredBytes = chain;
    return cube + chain;
}
int brmi_debug_env_lookup(const brmi_texture_desc* cubemaps, uint32_t cubemapCount, uint32_t cubemapIndex, const float* directions, const float* lods, float* outRGBA, uint32_t n, brmi_stream stream) {
    if (!cubemaps || !directions || !lods || !outRGBA) return BRMI_ERR_INVALID;
    if (n == 0u) return BRMI_OK;
    return brmi::launch_debug_env_lookup(cubemaps, cubemapCount, cubemapIndex, directions, lods, outRGBA, n, static_cast<hipStream_t>(stream));
}
// ---- texture mip chains (brmi_texmips.hip): every refusal comes before the first launch
static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0u; }
static uint32_t full_mip_count(uint32_t w, uint32_t h) { uint32_t n = 0u; for (uint32_t m = std::max(w, h); m; m >>= 1) n++; return n; }
static int texmips_refusal(const char* who, const brmi_texture_desc* t, const float* srgbToLinear) {
    if (!t) return stage_fail(BRMI_ERR_INVALID, "%s: the descriptor is null", who);
    if (!t->texels || !aligned4(t->texels)) return stage_fail(BRMI_ERR_INVALID, "%s: texels is null or not 4-byte aligned", who);
    if (!srgbToLinear || !aligned4(srgbToLinear)) return stage_fail(BRMI_ERR_INVALID, "%s: the sRGB decode table is null or not 4-byte aligned", who);
    if (t->format != BRMI_TEXTURE_FORMAT_RGBA8_UNORM && t->format != BRMI_TEXTURE_FORMAT_RGBA8_UNORM_SRGB)
        return stage_fail(BRMI_ERR_INVALID, "%s: format %u is neither RGBA8_UNORM nor RGBA8_UNORM_SRGB", who, t->format);
    if (t->width == 0u || t->height == 0u) return stage_fail(BRMI_ERR_INVALID, "%s: an empty image (%u x %u)", who, t->width, t->height);
    if (t->mipCount == 0u || t->mipCount > BRMI_TEXTURE_MAX_MIPS) return stage_fail(BRMI_ERR_INVALID, "%s: mipCount %u is outside [1, %u]", who, t->mipCount, BRMI_TEXTURE_MAX_MIPS);
    if (t->mipCount > full_mip_count(t->width, t->height))
        return stage_fail(BRMI_ERR_INVALID, "%s: mipCount %u, a %u x %u image has %u levels", who, t->mipCount, t->width, t->height, full_mip_count(t->width, t->height));
    for (uint32_t l = 0; l < t->mipCount; l++) {
        const uint64_t nl = (uint64_t)std::max(1u, t->width >> l) * std::max(1u, t->height >> l);
        if (t->mipOffset[l] + nl > 0x100000000ull) return stage_fail(BRMI_ERR_INVALID, "%s: level %u ends beyond what a 32-bit texel offset reaches", who, l);
        for (uint32_t k = 0; k < l; k++) {
            const uint64_t nk = (uint64_t)std::max(1u, t->width >> k) * std::max(1u, t->height >> k);
            if (t->mipOffset[l] < t->mipOffset[k] + nk && t->mipOffset[k] < t->mipOffset[l] + nl) return stage_fail(BRMI_ERR_INVALID, "%s: levels %u and %u overlap (mipOffset %u and %u)", who, k, l, t->mipOffset[k], t->mipOffset[l]);
        }
    }
    return BRMI_OK;
}
uint64_t brmi_texmips_bytes(uint32_t mipCount, uint64_t* scratchBytes, uint64_t* statsBytes, uint64_t* scalesBytes) {
    const bool ok = mipCount != 0u && mipCount <= BRMI_TEXTURE_MAX_MIPS;
    const uint64_t scratch = ok ? 4ull : 0ull, stats = ok ? 260ull * 4ull * mipCount : 0ull, scales = ok ? 4ull * mipCount : 0ull;
    if (scratchBytes) *scratchBytes = scratch; if (statsBytes) *statsBytes = stats; if (scalesBytes) *scalesBytes = scales;
    return scratch + stats + scales;
}
int brmi_texmips_build(const brmi_texture_desc* texture, const float* srgbToLinear, void* scratch, uint64_t scratchBytes, brmi_stream stream) {
    if (int rc = texmips_refusal("brmi_texmips_build", texture, srgbToLinear)) return rc;
    if (!scratch || !aligned4(scratch)) return stage_fail(BRMI_ERR_INVALID, "brmi_texmips_build: scratch is null or not 4-byte aligned");
    if (scratchBytes < 4u) return stage_fail(BRMI_ERR_CAPACITY, "brmi_texmips_build: scratch holds %llu bytes, brmi_texmips_bytes asks for 4", (unsigned long long)scratchBytes);
    if (texture->width > 4096u || texture->height > 4096u)
        return stage_fail(BRMI_ERR_CAPACITY, "brmi_texmips_build: %u x %u is beyond the 4096 texels one job reduces (the reference's job split is not built)", texture->width, texture->height);
    g_stageError.clear();
    if (texture->mipCount == 1u) return BRMI_OK;
    return brmi::launch_texmips_plain(*texture, srgbToLinear, static_cast<uint32_t*>(scratch), static_cast<hipStream_t>(stream));
}
int brmi_texmips_build_alpha(const brmi_texture_desc* texture, const float* srgbToLinear, uint32_t* stats, float* scales, brmi_stream stream) {
    if (int rc = texmips_refusal("brmi_texmips_build_alpha", texture, srgbToLinear)) return rc;
    if (!stats || !aligned4(stats) || !scales || !aligned4(scales)) return stage_fail(BRMI_ERR_INVALID, "brmi_texmips_build_alpha: stats or scales is null or not 4-byte aligned");
    g_stageError.clear();
    if (texture->mipCount == 1u) return BRMI_OK;
    return brmi::launch_texmips_alpha(*texture, srgbToLinear, stats, scales, static_cast<hipStream_t>(stream));
}
// ---- XeGTAO (brmi_gtao.hip): every refusal comes before the first launch
void brmi_gtao_default_settings(brmi_gtao_settings* s) {
    if (!s) return;
    *s = brmi_gtao_settings{};
    s->structSize = (uint32_t)sizeof(brmi_gtao_settings); s->qualityLevel = 2u; s->denoisePasses = 1u; s->radius = 0.5f; s->maxDepthLod = 0u;
}
int brmi_gtao_get_layout(uint32_t width, uint32_t height, brmi_gtao_layout* layout) {
    if (!layout || width == 0u || height == 0u) return BRMI_ERR_INVALID;
    brmi::gtao_layout(width, height, layout);
    return BRMI_OK;
}
int brmi_set_gtao(brmi_pass* p, const brmi_gtao_buffers* b) {
    if (!p) return BRMI_ERR_INVALID;
    if (!b) { p->gtao.on = false; p->gtao.b = brmi_gtao_buffers{}; return BRMI_OK; }
    if (b->structSize != sizeof(brmi_gtao_buffers)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_gtao: structSize %u, expected %zu", b->structSize, sizeof(brmi_gtao_buffers));
    const brmi_gtao_settings& st = b->settings;
    if (st.structSize != sizeof(brmi_gtao_settings)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_gtao: settings.structSize %u, expected %zu", st.structSize, sizeof(brmi_gtao_settings));
    // the taps of a pixel reach rows another GPU owns: no partition of the frame
    if (p->cfg.bandY0 != 0u || (p->cfg.bandY1 != 0u && p->cfg.bandY1 < p->cfg.height) || p->bandY0 != 0u || p->bandY1 < p->cfg.height || p->cfg.dynamicBand || p->stripes.count > 1u)
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_gtao: not with a row band, dynamicBand or the interleaved partition (a pixel's taps reach rows this GPU does not render)");
    if (st.qualityLevel > 3u) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_gtao: qualityLevel %u (0..3)", st.qualityLevel);
    if (st.denoisePasses > 3u) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_gtao: denoisePasses %u (0..3)", st.denoisePasses);
    if (!std::isfinite(st.radius) || !(st.radius > 0.0f)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_gtao: radius %g must be finite and > 0", (double)st.radius);
    if (st.maxDepthLod > 4u) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_gtao: maxDepthLod %u (0..4)", st.maxDepthLod);
    brmi_gtao_layout l; brmi::gtao_layout(p->cfg.width, p->cfg.height, &l);
    if (!b->scratch || !b->aoTerm) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_gtao: a null buffer");
    if ((reinterpret_cast<uintptr_t>(b->scratch) & 15u) || (reinterpret_cast<uintptr_t>(b->aoTerm) & 15u)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_gtao: scratch and aoTerm must be 16 B aligned");
    if (b->scratchBytes < l.scratchBytes) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_gtao: scratch holds %llu bytes, %u x %u pixels need %llu", (unsigned long long)b->scratchBytes, p->cfg.width, p->cfg.height, (unsigned long long)l.scratchBytes);
    if (b->aoTermBytes < l.outputBytes) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_gtao: aoTerm holds %llu bytes, %u x %u pixels need %llu", (unsigned long long)b->aoTermBytes, p->cfg.width, p->cfg.height, (unsigned long long)l.outputBytes);
    p->gtao.b = *b; p->gtao.layout = l; p->gtao.on = true;
    return BRMI_OK;
}
// what keeps a GTAO stage from running (host state only: brmi_execute_split asks before the frame's first launch)
static int gtao_refusal(brmi_pass* p, const char* what) {
    if (!p->setupDone || !p->updated) return brmi::fail(p, BRMI_ERR_STATE, "%s: setup/update not done", what);
    if (!p->gtao.on) return brmi::fail(p, BRMI_ERR_STATE, "%s: no GTAO buffers bound (brmi_set_gtao)", what);
    if (p->bandY0 != 0u || p->bandY1 < p->cfg.height) return brmi::fail(p, BRMI_ERR_STATE, "%s: the pass renders a row band", what);
    return BRMI_OK;
}
int brmi_gtao_prefilter(brmi_pass* p, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (int rc = gtao_refusal(p, "brmi_gtao_prefilter")) return rc;
    return brmi::launch_gtao_prefilter(p, static_cast<hipStream_t>(stream));
}
int brmi_gtao_main(brmi_pass* p, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (int rc = gtao_refusal(p, "brmi_gtao_main")) return rc;
    return brmi::launch_gtao_main(p, static_cast<hipStream_t>(stream));
}
int brmi_gtao_denoise(brmi_pass* p, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (int rc = gtao_refusal(p, "brmi_gtao_denoise")) return rc;
    return brmi::launch_gtao_denoise(p, static_cast<hipStream_t>(stream));
}
// ---- the display chain (brmi_display.hip): every refusal comes before the first launch
void brmi_display_default_settings(brmi_display_settings* s) {
    if (!s) return;
    *s = brmi_display_settings{};
    s->structSize = (uint32_t)sizeof(brmi_display_settings); s->tonemapType = 3u; s->bloom = 1u; s->autoExposure = 1u;
    s->minLogLuminance = brmi::display::kMinLogLuminance; s->logLuminanceRange = brmi::display::default_log_luminance_range();
    s->timeCoefficient = 1.0f / 60.0f; s->fixedAdaptedLuminance = 0.18f;
}
int brmi_display_get_layout(uint32_t width, uint32_t height, brmi_display_layout* layout) {
    if (!layout || width == 0u || height == 0u) return BRMI_ERR_INVALID;
    brmi::display_layout(width, height, layout);
    return BRMI_OK;
}
int brmi_set_display(brmi_pass* p, const brmi_display_buffers* b) {
    if (!p) return BRMI_ERR_INVALID;
    if (!b) { p->display.on = false; p->display.b = brmi_display_buffers{}; return BRMI_OK; }
    if (b->structSize != sizeof(brmi_display_buffers)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: structSize %u, expected %zu", b->structSize, sizeof(brmi_display_buffers));
    const brmi_display_settings& st = b->settings;
    if (st.structSize != sizeof(brmi_display_settings)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: settings.structSize %u, expected %zu", st.structSize, sizeof(brmi_display_settings));
    // the histogram is frame-wide and the bloom taps cross rows: no partition of the frame
    if (p->cfg.bandY0 != 0u || (p->cfg.bandY1 != 0u && p->cfg.bandY1 < p->cfg.height) || p->bandY0 != 0u || p->bandY1 < p->cfg.height || p->cfg.dynamicBand || p->stripes.count > 1u)
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: not with a row band, dynamicBand or the interleaved partition (the histogram is frame-wide, the bloom taps cross rows)");
    if (st.tonemapType > 4u) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: tonemapType %u (0..4)", st.tonemapType);
    if (st.bloom > 1u || st.autoExposure > 1u) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: bloom %u and autoExposure %u are 0 or 1", st.bloom, st.autoExposure);
    if (st.reserved[0] || st.reserved[1] || st.reserved[2] || st.reserved[3] || b->reserved) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: a reserved word is not zero");
    if (!std::isfinite(st.minLogLuminance) || !std::isfinite(st.logLuminanceRange) || !std::isfinite(st.timeCoefficient) || !std::isfinite(st.fixedAdaptedLuminance))
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: a setting is not finite");
    if (!(st.logLuminanceRange > 0.0f)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: logLuminanceRange %g must be > 0", (double)st.logLuminanceRange);
    if (st.bloom && !brmi::display::bloom_possible(p->cfg.width, p->cfg.height))
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: bloom needs 32 pixels a side, the frame is %u x %u (a level would have no rows)", p->cfg.width, p->cfg.height);
    brmi_display_layout l; brmi::display_layout(p->cfg.width, p->cfg.height, &l);
    if (!b->scratch || !b->ldr) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: a null buffer");
    if ((reinterpret_cast<uintptr_t>(b->scratch) & 15u) || (reinterpret_cast<uintptr_t>(b->blendedHdr) & 15u) || (reinterpret_cast<uintptr_t>(b->ldr) & 3u))
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: scratch and blendedHdr must be 16 B aligned, ldr 4 B");
    if (b->scratchBytes < l.scratchBytes) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: scratch holds %llu bytes, %u x %u pixels need %llu", (unsigned long long)b->scratchBytes, p->cfg.width, p->cfg.height, (unsigned long long)l.scratchBytes);
    if (b->ldrBytes < l.ldrBytes) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: ldr holds %llu bytes, %u x %u pixels need %llu", (unsigned long long)b->ldrBytes, p->cfg.width, p->cfg.height, (unsigned long long)l.ldrBytes);
    if (b->blendedHdr && b->blendedHdrBytes < l.blendedHdrBytes)
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_display: blendedHdr holds %llu bytes, %u x %u pixels need %llu", (unsigned long long)b->blendedHdrBytes, p->cfg.width, p->cfg.height, (unsigned long long)l.blendedHdrBytes);
    p->display.b = *b; p->display.layout = l; p->display.on = true;
    return BRMI_OK;
}
// what keeps a display stage from running (host state only: brmi_execute_split asks before the frame's first launch)
static int display_refusal(brmi_pass* p, const char* what) {
    if (!p->setupDone || !p->updated) return brmi::fail(p, BRMI_ERR_STATE, "%s: setup/update not done", what);
    if (!p->display.on) return brmi::fail(p, BRMI_ERR_STATE, "%s: no display buffers bound (brmi_set_display)", what);
    if (p->bandY0 != 0u || p->bandY1 < p->cfg.height) return brmi::fail(p, BRMI_ERR_STATE, "%s: the pass renders a row band", what);
    if (!p->res[BRMI_RES_HDR_COLOR]) return brmi::fail(p, BRMI_ERR_STATE, "%s: the HDR surface is not bound", what);
    return BRMI_OK;
}
int brmi_display_exposure(brmi_pass* p, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (int rc = display_refusal(p, "brmi_display_exposure")) return rc;
    return brmi::launch_display_exposure(p, static_cast<hipStream_t>(stream));
}
int brmi_display_bloom(brmi_pass* p, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (int rc = display_refusal(p, "brmi_display_bloom")) return rc;
    return brmi::launch_display_bloom(p, static_cast<hipStream_t>(stream));
}
int brmi_debug_display_histogram(brmi_pass* p, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (int rc = display_refusal(p, "brmi_debug_display_histogram")) return rc;
    if (!p->display.b.settings.autoExposure) return brmi::fail(p, BRMI_ERR_STATE, "brmi_debug_display_histogram: the binding has autoExposure off");
    return brmi::launch_display_exposure(p, static_cast<hipStream_t>(stream), true);
}
int brmi_debug_display_bloom_pass(brmi_pass* p, uint32_t mipIndex, uint32_t isUpsample, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (int rc = display_refusal(p, "brmi_debug_display_bloom_pass")) return rc;
    if (!p->display.b.settings.bloom) return brmi::fail(p, BRMI_ERR_STATE, "brmi_debug_display_bloom_pass: the binding has bloom off");
    if (isUpsample > 1u || mipIndex >= p->display.layout.bloomLevels || (isUpsample && mipIndex == 0u))
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_debug_display_bloom_pass: mipIndex %u, isUpsample %u (down 0..%u, up 1..%u)", mipIndex, isUpsample, p->display.layout.bloomLevels - 1u, p->display.layout.bloomLevels - 1u);
    return brmi::launch_display_bloom_pass(p, mipIndex, isUpsample != 0u, static_cast<hipStream_t>(stream));
}
int brmi_display_resolve(brmi_pass* p, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (int rc = display_refusal(p, "brmi_display_resolve")) return rc;
    return brmi::launch_display_resolve(p, static_cast<hipStream_t>(stream));
}
// ---- temporal anti-aliasing (brmi_temporal.hip): every refusal comes before the first launch
void brmi_temporal_default_settings(brmi_temporal_settings* s) {
    if (!s) return;
    *s = brmi_temporal_settings{};
    s->structSize = (uint32_t)sizeof(brmi_temporal_settings); s->blend = 0.1f; s->phases = 16u;
}
int brmi_temporal_get_layout(uint32_t width, uint32_t height, brmi_temporal_layout* layout) {
    if (!layout || width == 0u || height == 0u) return BRMI_ERR_INVALID;
    *layout = brmi_temporal_layout{};
    layout->historyBytes = brmi::temporal_image_bytes(width, height); layout->tilesX = (width + 7u) / 8u; layout->tilesY = (height + 7u) / 8u;
    return BRMI_OK;
}
// why the settings cannot be used (null: they can)
static const char* temporal_settings_refusal(const brmi_temporal_settings& st) {
    if (st.structSize != sizeof(brmi_temporal_settings)) return "settings.structSize is not sizeof(brmi_temporal_settings)";
    if (!std::isfinite(st.blend) || !(st.blend > 0.0f) || st.blend > 1.0f) return "blend must be finite and in (0, 1]";
    if (st.phases == 0u) return "phases is 0";
    for (uint32_t r : st.reserved) if (r) return "a reserved word is not zero";
    return nullptr;
}
int brmi_set_temporal(brmi_pass* p, const brmi_temporal_buffers* b) {
    if (!p) return BRMI_ERR_INVALID;
    if (!b) { p->temporal.on = false; p->temporal.b = brmi_temporal_buffers{}; p->temporal.valid = false; p->temporal.last = 1u; return BRMI_OK; }
    if (b->structSize != sizeof(brmi_temporal_buffers)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_temporal: structSize %u, expected %zu", b->structSize, sizeof(brmi_temporal_buffers));
    if (const char* why = temporal_settings_refusal(b->settings)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_temporal: %s", why);
    if (b->reserved) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_temporal: a reserved word is not zero");
    // a pixel's neighbourhood and its history taps reach rows another GPU owns: no partition of the frame
    if (p->cfg.bandY0 != 0u || (p->cfg.bandY1 != 0u && p->cfg.bandY1 < p->cfg.height) || p->bandY0 != 0u || p->bandY1 < p->cfg.height || p->cfg.dynamicBand || p->stripes.count > 1u)
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_temporal: not with a row band, dynamicBand or the interleaved partition (the neighbourhood and the history taps cross rows)");
    if (p->history || !p->historyUsers.empty())
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_temporal: the pass is linked to another by brmi_set_history_source (each pass would hold every second frame's history)");
    const uint64_t need = brmi::temporal_image_bytes(p->cfg.width, p->cfg.height);
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(b->history[0]), a1 = reinterpret_cast<uintptr_t>(b->history[1]);
    if (!a0 || !a1) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_temporal: a null image");
    if ((a0 & 15u) || (a1 & 15u)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_temporal: the images must be 16 B aligned");
    if (b->historyBytes < need) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_temporal: an image holds %llu bytes, %u x %u pixels need %llu", (unsigned long long)b->historyBytes, p->cfg.width, p->cfg.height, (unsigned long long)need);
    if (a0 < a1 + need && a1 < a0 + need) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_temporal: the two images overlap");
    p->temporal.b = *b; p->temporal.on = true; p->temporal.valid = false; p->temporal.last = 1u;      // (the first resolve writes image 0)
    return BRMI_OK;
}
// what keeps the temporal stage from running (host state only: brmi_execute_split asks before the frame's first launch)
static int temporal_refusal(brmi_pass* p, const char* what) {
    if (!p->setupDone || !p->updated) return brmi::fail(p, BRMI_ERR_STATE, "%s: setup/update not done", what);
    if (!p->temporal.on) return brmi::fail(p, BRMI_ERR_STATE, "%s: no history images bound (brmi_set_temporal)", what);
    if (p->bandY0 != 0u || p->bandY1 < p->cfg.height) return brmi::fail(p, BRMI_ERR_STATE, "%s: the pass renders a row band", what);
    if (!p->res[BRMI_RES_HDR_COLOR] || !p->res[BRMI_RES_LINEAR_DEPTH] || !p->res[BRMI_RES_GBUF_MOTION_VECTORS]) return brmi::fail(p, BRMI_ERR_STATE, "%s: the HDR, depth or motion-vector surface is not bound", what);
    return BRMI_OK;
}
int brmi_temporal_resolve(brmi_pass* p, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (int rc = temporal_refusal(p, "brmi_temporal_resolve")) return rc;
    return brmi::launch_temporal_resolve(p, static_cast<hipStream_t>(stream));
}
int brmi_temporal_reset(brmi_pass* p) {
    if (!p) return BRMI_ERR_INVALID;
    if (!p->temporal.on) return brmi::fail(p, BRMI_ERR_STATE, "brmi_temporal_reset: no history images bound (brmi_set_temporal)");
    p->temporal.valid = false;
    return BRMI_OK;
}
int brmi_temporal_state(const brmi_pass* p, uint32_t* resolvedIndex, uint32_t* historyValid) {
    if (!p || !p->temporal.on) return p ? BRMI_ERR_STATE : BRMI_ERR_INVALID;
    if (resolvedIndex) *resolvedIndex = p->temporal.last;
    if (historyValid) *historyValid = p->temporal.valid ? 1u : 0u;
    return BRMI_OK;
}
int brmi_debug_temporal_resolve(uint32_t width, uint32_t height, const void* hdr, const void* depth, const void* motion, const void* history, void* out,
                                const brmi_temporal_settings* settings, brmi_stream stream) {
    if (width == 0u || height == 0u || width > 65536u || height > 65536u) return stage_fail(BRMI_ERR_INVALID, "brmi_debug_temporal_resolve: a frame of %u x %u pixels", width, height);
    if (!hdr || !depth || !motion || !out || !settings) return stage_fail(BRMI_ERR_INVALID, "brmi_debug_temporal_resolve: a null surface or null settings");
    if ((reinterpret_cast<uintptr_t>(hdr) & 7u) || (reinterpret_cast<uintptr_t>(history) & 7u) || (reinterpret_cast<uintptr_t>(out) & 7u) || !aligned4(depth) || !aligned4(motion))
        return stage_fail(BRMI_ERR_INVALID, "brmi_debug_temporal_resolve: hdr, history and out must be 8 B aligned, depth and motion 4 B");
    if (out == hdr || out == history) return stage_fail(BRMI_ERR_INVALID, "brmi_debug_temporal_resolve: out is one of the inputs");
    if (const char* why = temporal_settings_refusal(*settings)) return stage_fail(BRMI_ERR_INVALID, "brmi_debug_temporal_resolve: %s", why);
    g_stageError.clear();
    const hipError_t e = brmi::launch_temporal_surfaces(width, height, hdr, depth, motion, history, out, settings->blend, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? BRMI_OK : stage_fail(BRMI_ERR_HIP, "launch k_temporal_resolve: %s", hipGetErrorString(e));
}
int brmi_streaming_feedback(brmi_pass* p, brmi_stream stream) {
    CHECK_READY(p);
    if (!p->streaming.on) return brmi::fail(p, BRMI_ERR_STATE, "brmi_streaming_feedback: no streaming buffers bound (brmi_set_streaming)");
    return brmi::launch_streaming_feedback(p, static_cast<hipStream_t>(stream));
}
uint64_t brmi_debug_view_bytes(uint32_t width, uint32_t height) { return (uint64_t)((width + 7u) / 8u) * ((height + 7u) / 8u) * 64u * 8u; }
int brmi_set_debug_view(brmi_pass* p, const brmi_debug_view_buffers* b) {
    if (!p) return BRMI_ERR_INVALID;
    if (!b) { p->debugView.on = false; return BRMI_OK; }
    if (b->structSize != sizeof(brmi_debug_view_buffers)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_debug_view: structSize %u, expected %zu", b->structSize, sizeof(brmi_debug_view_buffers));
    if (p->stripes.count > 1u) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_debug_view: not with the interleaved partition (stripeCount %u): the compact surfaces' pixel rows are not the frame's", p->stripes.count);
    if (!b->payload) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_debug_view: the payload pointer is null");
    if (reinterpret_cast<uintptr_t>(b->payload) & 15u) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_debug_view: the payload must be 16 B aligned");
    const uint64_t need = brmi_debug_view_bytes(p->cfg.width, p->cfg.height), needImage = (uint64_t)p->cfg.width * p->cfg.height * 4u;
    if (b->payloadBytes < need) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_debug_view: the payload holds %llu bytes, %u x %u pixels need %llu", (unsigned long long)b->payloadBytes, p->cfg.width, p->cfg.height, (unsigned long long)need);
    if (b->image && ((reinterpret_cast<uintptr_t>(b->image) & 3u) || b->imageBytes < needImage))
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_debug_view: the image holds %llu bytes (4 B aligned), %u x %u pixels need %llu", (unsigned long long)b->imageBytes, p->cfg.width, p->cfg.height, (unsigned long long)needImage);
    p->debugView.b = *b; p->debugView.on = true;
    return BRMI_OK;
}
// Why the pass cannot write the view perFrame.outputType asks for (0: it can).  Host state only: brmi_execute_split asks BEFORE it launches anything, so a
// refused mode leaves no half-issued frame behind.
static int debug_view_refusal(brmi_pass* p) {
    const uint32_t mode = p->pfHost.outputType;
    if (!brmi::debug_view_mode_built(mode)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_debug_view: outputType %u is not a debug view of this path (brmi_output_type lists the ones it builds)", mode);
    if ((mode == BRMI_OUTPUT_LIGHT_CLUSTER_ID || mode == BRMI_OUTPUT_LIGHT_CLUSTER_LIGHT_COUNT) && !p->cfg.enableClusteredLighting)
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_debug_view: outputType %u needs enableClusteredLighting", mode);
    if (!p->debugView.on) return brmi::fail(p, BRMI_ERR_STATE, "brmi_debug_view: no debug target bound (brmi_set_debug_view)");
    if (p->stripes.count > 1u) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_debug_view: not with the interleaved partition");
    return BRMI_OK;
}
int brmi_debug_view(brmi_pass* p, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (!p->setupDone) return brmi::fail(p, BRMI_ERR_STATE, "brmi_debug_view: call brmi_setup first");
    if (!p->updated) return brmi::fail(p, BRMI_ERR_STATE, "brmi_debug_view: call brmi_update first (the view is perFrame.outputType of the last update)");
    if (p->pfHost.outputType == BRMI_OUTPUT_COLOR) return BRMI_OK;
    if (int rc = debug_view_refusal(p)) return rc;
    return brmi::launch_debug_view(p, static_cast<hipStream_t>(stream));
}
int brmi_build_hzb(brmi_pass* p, brmi_stream stream) {
    CHECK_READY(p); brmi::FrameCtx ctx;
    if (!p->cfg.enableOcclusionCulling) return brmi::fail(p, BRMI_ERR_STATE, "brmi_build_hzb: the pass was created without enableOcclusionCulling");
    return stage_hzb(p, ctx, stream, brmi::ChainBuild::FromDepthMap);
}
int brmi_invalidate_hzb(brmi_pass* p) {
    if (!p) return BRMI_ERR_INVALID;
    p->hzbValid = false;
    if (p->history) p->history->hzbValid = false;      // the chain the next phase 1 would test against is the source's
    return BRMI_OK;
}
int brmi_set_history_source(brmi_pass* p, brmi_pass* source) {
    if (!p) return BRMI_ERR_INVALID;
    if (source == p) source = nullptr;
    if (source) {
        if (p->temporal.on || source->temporal.on) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_history_source: not with a temporal binding (brmi_set_temporal) on either pass");
        if (!p->setupDone || !source->setupDone) return brmi::fail(p, BRMI_ERR_STATE, "brmi_set_history_source: both passes need brmi_setup first");
        if (!p->cfg.enableOcclusionCulling || !source->cfg.enableOcclusionCulling) return brmi::fail(p, BRMI_ERR_STATE, "brmi_set_history_source: both passes need enableOcclusionCulling (there is no history otherwise)");
        if (p->cfg.width != source->cfg.width || p->cfg.height != source->cfg.height || ((p->bandY0 != source->bandY0 || p->bandY1 != source->bandY1) && !(p->cfg.dynamicBand && source->cfg.dynamicBand)))
            return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_history_source: the passes differ in size or band (%ux%u rows %u-%u against %ux%u rows %u-%u)", p->cfg.width, p->cfg.height, p->bandY0, p->bandY1,
                              source->cfg.width, source->cfg.height, source->bandY0, source->bandY1);
    }
    if (p->history) { auto& u = p->history->historyUsers; u.erase(std::remove(u.begin(), u.end(), p), u.end()); }
    p->history = source;
    if (source) source->historyUsers.push_back(p);
    return BRMI_OK;
}
int brmi_gbuffer(brmi_pass* p, brmi_stream stream) { CHECK_READY(p); brmi::FrameCtx ctx; return stage_gbuffer(p, ctx, stream); }
int brmi_light_clustering(brmi_pass* p, brmi_stream stream) { CHECK_READY(p); brmi::FrameCtx ctx; return stage_light_clustering(p, ctx, stream); }
int brmi_set_shade_slabs(brmi_pass* p, uint32_t slabs, brmi_slab_fn fn, void* user) {
    if (!p) return BRMI_ERR_INVALID;
    p->shadeSlabs = (fn && slabs > 1u) ? slabs : 0u; p->shadeSlabFn = p->shadeSlabs ? fn : nullptr; p->shadeSlabUser = p->shadeSlabs ? user : nullptr;
    return BRMI_OK;
}
int brmi_shade(brmi_pass* p, brmi_stream stream) { CHECK_READY(p); brmi::FrameCtx ctx; return stage_shade(p, ctx, stream); }

// The whole chain in graph order.  K6 is folded into the G-buffer kernel (one visibility read).
int brmi_execute(brmi_pass* p, brmi_stream stream) { return brmi_execute_split(p, stream, stream); }

// Geometry half (culling, rasterisation, depth chain: latency-bound launches that leave most of the chip idle) on `stream`, resolve +
// shading half (VALU-bound, fills the chip) on `shadeStream`.  With two linked passes alternating frames on the SAME two streams -- the
// geometry stream created with a higher priority -- frame k+1's geometry runs beside frame k's shading and gets CU slots first.
int brmi_execute_split(brmi_pass* p, brmi_stream stream, brmi_stream shadeStream) {
    CHECK_READY(p);
    int rc;
    // a debug view the pass cannot write is refused here, before the frame's first launch and before any of its bookkeeping
    const bool debugView = p->debugView.on && p->pfHost.outputType != BRMI_OUTPUT_COLOR;
    if (debugView && (rc = debug_view_refusal(p))) return rc;
    const bool skybox = p->env.on && p->env.b.skybox;      // ... and so is a skybox stage that could not run
    if (skybox && (rc = skybox_refusal(p))) return rc;
    if (p->gtao.on && (rc = gtao_refusal(p, "brmi_execute"))) return rc;      // ... and the GTAO stages of a bound term
    if (p->temporal.on && (rc = temporal_refusal(p, "brmi_execute"))) return rc;      // ... and the temporal resolve of bound history images
    if (p->display.on && (rc = display_refusal(p, "brmi_execute"))) return rc;      // ... and the display chain of a bound target
    p->executesSinceTimes++;
    const bool split = shadeStream != stream;
    if ((rc = wait_for_frames_in_flight(p, stream))) return rc;      // (once for the frame: the stage bodies below have none)
    // When the phase-1 traversal is the one-launch LDS walk and the frame constants are due anyway, the frame needs no clear launch: the
    // constants kernel zeroes the culling state and the walk's launch carries the visibility clear (brmi_cull.hip, SideClear).
    const bool rides = p->constantsSerial != p->updateSerial && p->tables.minLevelWidth <= 1024u /* the one-launch walk runs (brmi_cull.hip: HIER_CAP_MAX) */ && !p->forceLevelKernels && p->scene.activeDrawCount != 0u;
    // A split frame (round 4): the riders move to where they fit -- the visibility clear onto k_cull_clusters' launch (brmi_cull.hip: ClearRide), the
    // light clustering onto the shading stream, which is idle until this frame's pixel pass (below, behind the same event as the early resolve setup).
    const bool sideRiders = rides && split && (p->bandPixelCount & 1ull) == 0ull;
    // the frame's plan: every fused form it asks of the launchers, here and nowhere else (brmi_internal.h: FrameCtx, whose second half they answer in)
    brmi::FrameCtx ctx;
    ctx.twoStreams = split;
    ctx.visibilityClear = sideRiders ? brmi::VisibilityClear::OnClusterCull : (rides ? brmi::VisibilityClear::OnTraversal : brmi::VisibilityClear::OwnLaunch);
    ctx.constantsClearFrameState = rides; ctx.clearTakesFrameState = !rides;
    ctx.depthIsFinal = p->cfg.enableOcclusionCulling != 0;      // (both chain builds below come before the G-buffer kernel)
    if (!rides && (rc = stage_clear(p, ctx, stream))) return rc;
    if ((rc = stage_cull(p, ctx, 1, stream))) return rc;
    if (!ctx.visibilityCleared) return brmi::fail(p, BRMI_ERR_STATE, sideRiders ? "brmi_execute: the cluster culling did not carry the visibility clear" : "brmi_execute: the traversal did not carry the visibility clear");
    // The per-cluster resolve tables need the cluster list, not the keys: for the phase-1 clusters they are made NOW, on the shading stream (idle until
    // this frame's pixel pass), beside the rasteriser -- the geometry half is a chain of latency-bound launches and this one was 40 us at its end.
    // (Not on frames of more triangles than pixels, whose setup skips clusters that own no pixel and so needs the final keys; a frame that resolves
    // without tables launches nothing there: launch_resolve_setup.)
    if (split) {
        if (!p->cullDone) BRMI_HIP(p, hipEventCreateWithFlags(&p->cullDone, hipEventDisableTiming));
        BRMI_HIP(p, hipEventRecord(p->cullDone, static_cast<hipStream_t>(stream)));
        BRMI_HIP(p, hipStreamWaitEvent(static_cast<hipStream_t>(shadeStream), p->cullDone, 0));
        if (sideRiders && (rc = brmi::launch_light_clustering(p, ctx, static_cast<hipStream_t>(shadeStream)))) return rc;
        if ((rc = launch_resolve_setup(p, ctx, static_cast<hipStream_t>(shadeStream), 1u))) return rc;
    }
    if ((rc = stage_raster(p, ctx, 1, stream))) return rc;
    if (p->cfg.enableOcclusionCulling) {
        // reference graph: LinearDepthCopyPass1 -> LinearDepthDownsamplePass1 -> HierarchicalCullingPass2 -> ...RasterizeClustersPass2
        // -> LinearDepthCopyPass2 -> LinearDepthDownsamplePass2 (CLodExtension.cpp:1920-2088); the first build's tail seeds phase 2
        if ((rc = stage_hzb(p, ctx, stream, brmi::ChainBuild::AfterPhase1))) return rc;
        if ((rc = stage_cull(p, ctx, 2, stream))) return rc;
        if ((rc = stage_raster(p, ctx, 2, stream))) return rc;
        // LinearDepthCopyPass2 + LinearDepthDownsamplePass2 straight from the final visibility keys, skipped on the device when phase 2 drew
        // nothing: the depth map and the chain are final BEFORE the G-buffer kernel (which then skips its depth store), so a pass that
        // renders the next frame on another stream (brmi_set_history_source) can start while this frame is resolved and shaded.
        if ((rc = stage_hzb(p, ctx, stream, brmi::ChainBuild::AfterPhase2))) return rc;
        // recorded every frame (a pass may be linked to this one later, from another stream)
        if (!p->chainReady) BRMI_HIP(p, hipEventCreateWithFlags(&p->chainReady, hipEventDisableTiming));
        BRMI_HIP(p, hipEventRecord(p->chainReady, static_cast<hipStream_t>(stream)));
        p->chainRecorded = true; p->chainStream = stream;
    }
    // CLodStreamingFeedbackSortPass, behind the frame's last culling phase on the geometry stream (behind the chain event: a linked pass's next frame does not wait for it)
    if (p->streaming.on && (rc = brmi_streaming_feedback(p, stream))) return rc;
    if (split) {
        if ((rc = launch_resolve_setup(p, ctx, static_cast<hipStream_t>(stream), 2u))) return rc;      // (with part 1 above: the G-buffer stage finds its tables made)
        if (!p->geometryDone) BRMI_HIP(p, hipEventCreateWithFlags(&p->geometryDone, hipEventDisableTiming));
        if (!p->frameDone) BRMI_HIP(p, hipEventCreateWithFlags(&p->frameDone, hipEventDisableTiming));
        BRMI_HIP(p, hipEventRecord(p->geometryDone, static_cast<hipStream_t>(stream)));
        BRMI_HIP(p, hipStreamWaitEvent(static_cast<hipStream_t>(shadeStream), p->geometryDone, 0));
        stream = shadeStream;
    }
    if ((rc = stage_gbuffer(p, ctx, stream))) return rc;
    if (!ctx.lightGridBuilt && (rc = stage_light_clustering(p, ctx, stream))) return rc;      // (not where the culling pass's launches, or the shading stream beside them, carried it)
    // BuildGTAOPipeline between the G-buffer and the deferred shading, on the shading stream, inside the shading stage's event pair (brmi_stage does not grow)
    if ((rc = stage_shade(p, ctx, stream, p->gtao.on))) return rc;
    // SkyboxRenderPass behind the deferred shading (the reference's Deferred -> Skybox -> Forward), only where the bound environment asks for it
    if (skybox && (rc = brmi_skybox(p, stream))) return rc;
    // the temporal resolve where the reference runs its upscaler: behind the skybox, ahead of the display chain, which then reads the resolved image
    if (p->temporal.on && (rc = brmi::launch_temporal_resolve(p, static_cast<hipStream_t>(stream)))) return rc;
    // LuminanceHistogram(+Average)Pass, BuildBloomPipeline and TonemappingPass behind the lit frame, on the shading stream, in front of the frame's end
    if (p->display.on) {
        hipStream_t ds = static_cast<hipStream_t>(stream);
        if ((rc = brmi::launch_display_exposure(p, ds)) || (rc = brmi::launch_display_bloom(p, ds)) || (rc = brmi::launch_display_resolve(p, ds))) return rc;
    }
    // the debug payload of perFrame.outputType, from the surfaces the frame has just made (behind the shading stage, on its stream, in front of the frame's end)
    if (debugView && (rc = brmi_debug_view(p, stream))) return rc;
    if (split) { BRMI_HIP(p, hipEventRecord(p->frameDone, static_cast<hipStream_t>(stream))); p->frameDoneRecorded = true; }
    return BRMI_OK;
}

int brmi_read_counters(brmi_pass* p, brmi_counters* out, brmi_stream stream) {
    if (!p || !out) return BRMI_ERR_INVALID;
    if (!p->setupDone) return brmi::fail(p, BRMI_ERR_STATE, "brmi_read_counters: setup not done");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t c[CNT_WORDS];
    BRMI_HIP(p, hipMemcpyAsync(c, p->counters(), sizeof(c), hipMemcpyDeviceToHost, s));
    BRMI_HIP(p, hipStreamSynchronize(s));
    std::memset(out, 0, sizeof(*out));
    out->instancesTested = c[CNT_INSTANCES_TESTED]; out->instancesVisible = c[CNT_INSTANCES_VISIBLE];
    out->nodesVisited = c[CNT_NODES_VISITED];
    uint32_t overflowQueued = 0;
    for (uint32_t st = 0; st < CNT_STRIPE_COUNT; st++) {
        const uint32_t* sp = c + CNT_STRIPES + st * CNT_STRIPE_WORDS;
        out->instancesTested += sp[0]; out->instancesVisible += sp[1]; out->nodesVisited += sp[2];
        overflowQueued += sp[STRIPE_OVERFLOW];
    } out->bucketRecords = c[CNT_BUCKETS]; out->meshletsTested = c[CNT_MESHLETS_TESTED];
    for (uint32_t st = 0; st < CNT_STRIPE_COUNT; st++) out->meshletsTested += c[CNT_STRIPES + st * CNT_STRIPE_WORDS + STRIPE_MESHLETS_TESTED];
    out->visibleClusters = c[CNT_VISIBLE]; out->visibleClustersPhase2 = c[CNT_VISIBLE2];
    out->droppedRecords = c[CNT_DROPPED_RECORDS]; out->droppedClusters = c[CNT_DROPPED_CLUSTERS]; out->lightPagesUsed = c[CNT_LIGHT_PAGES];
    out->reserved[0] = c[CNT_SUM_VERTS_LO]; out->reserved[2] = c[CNT_SUM_VERTS_HI];      // (vertex sum | triangle sum << 32 in one word, brmi_internal.h)
    out->reserved[1] = std::min(c[CNT_HELD1], p->cfg.maxVisibleClusters); out->reserved[3] = std::min(c[CNT_LATE1], p->cfg.maxVisibleClusters);      // round 6: the draw list (include/brmi.h)
    out->reserved[4] = c[CNT_RASTER_CLUSTERS]; out->reserved[5] = c[CNT_BIN_OVERFLOW] + overflowQueued;
    out->replayNodes = c[CNT_REPLAY_NODES]; out->replayMeshlets = c[CNT_REPLAY_MESHLETS];
    return BRMI_OK;
}

int brmi_set_timed_stages(brmi_pass* p, uint32_t stageMask) {
    if (!p) return BRMI_ERR_INVALID;
    p->timedStages = stageMask;
    return BRMI_OK;
}

int brmi_stage_times(brmi_pass* p, float* ms) {
    if (!p || !ms) return BRMI_ERR_INVALID;
    if (!p->eventsCreated) return brmi::fail(p, BRMI_ERR_STATE, "brmi_stage_times: collectPassStatistics is off");
    // mean PER FRAME over the recordings since the previous call (at most the last kEventRing), then reset.  brmi_execute records the
    // depth-chain stage twice per frame (before phase 2 and after the G-buffer pass): its two recordings are one frame's cost.
    for (int i = 0; i < BRMI_STAGE_COUNT; i++) {
        ms[i] = 0.0f;
        const uint32_t perFrame = (i == BRMI_STAGE_HZB && p->executesSinceTimes != 0u && p->evCount[i] == 2u * p->executesSinceTimes) ? 2u : 1u;
        uint32_t n = std::min(p->evCount[i], brmi_pass::kEventRing);
        n -= n % perFrame;
        if (n == 0) continue;
        double sum = 0.0;
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t slot = (p->evCount[i] - 1 - k) % brmi_pass::kEventRing;
            float t = 0.0f;
            BRMI_HIP(p, hipEventSynchronize(p->evStop[i][slot]));
            BRMI_HIP(p, hipEventElapsedTime(&t, p->evStart[i][slot], p->evStop[i][slot]));
            sum += t;
        }
        ms[i] = (float)(sum / (n / perFrame));
        p->evCount[i] = 0;
    }
    p->executesSinceTimes = 0;
    return BRMI_OK;
}

// bytes_frame = 140*P + sum_clusters(144 + 12V + 3T) + 64*M_tested + 16*M_visible + 64*N_nodes
int brmi_algorithmic_bytes(brmi_pass* p, uint64_t* perStage, uint64_t* total) {
    if (!p || !perStage || !total) return BRMI_ERR_INVALID;
    // a read-back call: waits for whatever stream the frame was executed on (a non-blocking stream does not order with the NULL stream)
    BRMI_HIP(p, hipDeviceSynchronize());
    brmi_counters c; int rc = brmi_read_counters(p, &c, nullptr); if (rc) return rc;
    const uint64_t P = (uint64_t)p->cfg.width * (p->bandY1 - p->bandY0);
    uint64_t sumV = c.reserved[0], sumT = c.reserved[2], nClusters = c.reserved[4];
    if (c.reserved[1] != 0u) {      // a frame that held clusters back: what was rasterised is the draw list, the late list and phase 2 (the held clusters that stayed hidden moved no vertex or index byte)
        uint32_t vt[2];
        BRMI_HIP(p, hipMemcpy(vt, p->counters() + CNT_DRAWN_VT, 8, hipMemcpyDeviceToHost));
        sumV = vt[0]; sumT = vt[1]; nClusters -= c.reserved[1] - c.reserved[3];
    }
    for (int i = 0; i < BRMI_STAGE_COUNT; i++) perStage[i] = 0;
    perStage[BRMI_STAGE_CLEAR] = 8 * P;
    perStage[BRMI_STAGE_CULL] = 64ull * c.meshletsTested + 16ull * (c.visibleClusters + c.visibleClustersPhase2) + 64ull * c.nodesVisited;
    perStage[BRMI_STAGE_RASTER] = 8 * P + 144ull * nClusters + 12ull * sumV + 3ull * sumT;
    if (p->cfg.enableOcclusionCulling) {
        // depth copy: 8 B key in, 4 B depth out; chain: every depth texel read once, 1/3 of that written, built twice per frame;
        // phase-2 cull / raster traffic is counted in the cull / raster rows (their counters accumulate over both phases)
        perStage[BRMI_STAGE_DEPTH_COPY] = 12 * P;
        perStage[BRMI_STAGE_HZB] = 2 * (4 * P + 4 * P / 3);
    }
    perStage[BRMI_STAGE_GBUFFER] = (8 + 52 + 4) * P;
    perStage[BRMI_STAGE_SHADE] = (4 + 48 + 8) * P;
    *total = 0; for (int i = 0; i < BRMI_STAGE_COUNT; i++) *total += perStage[i];
    return BRMI_OK;
}

int brmi_algorithmic_bytes_launched(brmi_pass* p, uint64_t* perStage, uint64_t* total) {
    if (int rc = brmi_algorithmic_bytes(p, perStage, total)) return rc;
    if (!p->tables.hasCoat && !p->tables.hasFuzz) {      // k_shade<0>: depth 4 + normals 16 + albedo 4 + metallic / roughness 4 + emissive 8 read, HDR 8 written; the coat and fuzz planes (8 + 8) stay unread
        const uint64_t P = (uint64_t)p->cfg.width * (p->bandY1 - p->bandY0);
        *total -= perStage[BRMI_STAGE_SHADE]; perStage[BRMI_STAGE_SHADE] = 44ull * P; *total += perStage[BRMI_STAGE_SHADE];
    }
    return BRMI_OK;
}

int brmi_debug_read_held(brmi_pass* p, uint32_t* held, uint32_t heldCapacity, uint32_t* heldCount, uint32_t* late, uint32_t lateCapacity, uint32_t* lateCount) {
    if (!p || !heldCount || !lateCount || !p->setupDone) return BRMI_ERR_INVALID;
    BRMI_HIP(p, hipDeviceSynchronize());
    uint32_t nh = 0, nl = 0;
    BRMI_HIP(p, hipMemcpy(&nh, p->counters() + CNT_HELD1, 4, hipMemcpyDeviceToHost));
    BRMI_HIP(p, hipMemcpy(&nl, p->counters() + CNT_LATE1, 4, hipMemcpyDeviceToHost));
    if (!p->holdEnabled) nh = nl = 0;
    nh = std::min(nh, p->cfg.maxVisibleClusters); nl = std::min(nl, p->cfg.maxVisibleClusters);
    *heldCount = nh; *lateCount = nl;
    if (held && nh) {
        std::vector<HeldRecord> rec(std::min(nh, heldCapacity));
        if (!rec.empty()) BRMI_HIP(p, hipMemcpy(rec.data(), p->wsPtr<HeldRecord>(p->ws.heldRecords), rec.size() * sizeof(HeldRecord), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < rec.size(); i++) held[i] = rec[i].clusterIndex;
    }
    if (late && nl && lateCapacity) BRMI_HIP(p, hipMemcpy(late, p->wsPtr<uint32_t>(p->ws.lateList), (size_t)std::min(nl, lateCapacity) * 4, hipMemcpyDeviceToHost));
    return BRMI_OK;
}

int brmi_debug_read_draw_list(brmi_pass* p, uint32_t* draw, uint32_t drawCapacity, uint32_t* drawCount, uint32_t* heldBoxes, uint32_t heldCapacity, uint32_t* heldCount, uint32_t* boxCount) {
    if (!p || !drawCount || !heldCount || !p->setupDone) return BRMI_ERR_INVALID;
    BRMI_HIP(p, hipDeviceSynchronize());
    uint32_t nd = 0, nh = 0;      // (as the kernel left them: a count beyond the list's capacity is the caller's to see)
    BRMI_HIP(p, hipMemcpy(&nd, p->counters() + CNT_DRAW1, 4, hipMemcpyDeviceToHost));
    BRMI_HIP(p, hipMemcpy(&nh, p->counters() + CNT_HELD1, 4, hipMemcpyDeviceToHost));
    if (!p->holdEnabled) nd = nh = 0;
    *drawCount = nd; *heldCount = nh;
    if (boxCount) *boxCount = p->tables.totalBoxes;
    const uint32_t rd = std::min(std::min(nd, drawCapacity), p->cfg.maxVisibleClusters), rh = std::min(std::min(nh, heldCapacity), p->cfg.maxVisibleClusters);
    if (draw && rd) BRMI_HIP(p, hipMemcpy(draw, p->wsPtr<uint32_t>(p->ws.drawList), (size_t)rd * 4, hipMemcpyDeviceToHost));
    if (heldBoxes && rh) {
        std::vector<HeldRecord> rec(rh);
        BRMI_HIP(p, hipMemcpy(rec.data(), p->wsPtr<HeldRecord>(p->ws.heldRecords), rec.size() * sizeof(HeldRecord), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < rec.size(); i++) heldBoxes[i] = rec[i].boxIndex;
    }
    return BRMI_OK;
}

int brmi_debug_wide_triangles(brmi_pass* p, uint32_t out[3]) {
    if (!p || !out || !p->setupDone) return BRMI_ERR_INVALID;
    BRMI_HIP(p, hipDeviceSynchronize());
    uint32_t c[3] = {0u, 0u, 0u};
    BRMI_HIP(p, hipMemcpy(&c[0], p->counters() + CNT_WIDE1, 4, hipMemcpyDeviceToHost));
    BRMI_HIP(p, hipMemcpy(&c[1], p->counters() + CNT_WIDE1B, 4, hipMemcpyDeviceToHost));
    BRMI_HIP(p, hipMemcpy(&c[2], p->counters() + CNT_WIDE2, 4, hipMemcpyDeviceToHost));
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
    return BRMI_OK;
}

int brmi_debug_lean_clusters(brmi_pass* p, uint32_t out[4]) {
    if (!p || !out || !p->setupDone) return BRMI_ERR_INVALID;
    BRMI_HIP(p, hipDeviceSynchronize());
    uint32_t c = 0u, heads[64 * 32];
    BRMI_HIP(p, hipMemcpy(&c, p->counters() + CNT_GENERAL1, 4, hipMemcpyDeviceToHost));
    BRMI_HIP(p, hipMemcpy(heads, p->counters() + CNT_BIG1, sizeof(heads), hipMemcpyDeviceToHost));
    out[0] = p->leanLastLaunch ? 1u : 0u; out[1] = c; out[2] = out[3] = 0u;
    for (uint32_t s = 0; s < 64u; s++) { out[2] += heads[s * 32u]; out[3] += heads[s * 32u + 1u]; }
    return BRMI_OK;
}

int brmi_debug_raster_shape(brmi_pass* p, uint32_t* slim) {
    if (!p || !slim || !p->setupDone) return BRMI_ERR_INVALID;
    *slim = p->slimLastLaunch ? 1u : 0u;
    return BRMI_OK;
}

int brmi_debug_read_lean_queue(brmi_pass* p, uint32_t stripe, uint32_t* runs, uint32_t maxRuns, void* entries, uint32_t maxEntries, uint32_t counts[2]) {
    if (!p || !counts || !p->setupDone || stripe >= 64u || p->leanMinClusters == 0u) return BRMI_ERR_INVALID;
    BRMI_HIP(p, hipDeviceSynchronize());
    uint32_t head[2];
    BRMI_HIP(p, hipMemcpy(head, p->counters() + CNT_BIG1 + stripe * 32u, 8, hipMemcpyDeviceToHost));
    const uint32_t cap = p->leanQueue / 64u;
    counts[0] = std::min(head[0], cap); counts[1] = std::min(head[1], cap);
    if (runs) BRMI_HIP(p, hipMemcpy(runs, p->wsPtr<uint8_t>(p->ws.bigRuns) + (size_t)stripe * cap * 8u, (size_t)std::min(maxRuns, counts[1]) * 8u, hipMemcpyDeviceToHost));
    if (entries) BRMI_HIP(p, hipMemcpy(entries, p->wsPtr<uint8_t>(p->ws.bigQueue) + (size_t)stripe * cap * 96u, (size_t)std::min(maxEntries, counts[0]) * 96u, hipMemcpyDeviceToHost));
    return BRMI_OK;
}

int brmi_debug_read_bin_records(brmi_pass* p, void* dst, uint64_t bytes) {
    if (!p || !dst || !p->setupDone) return BRMI_ERR_INVALID;
    BRMI_HIP(p, hipDeviceSynchronize());
    if ((bytes >> 62) & 1ull) { bytes &= ~(1ull << 62); BRMI_HIP(p, hipMemset(p->wsPtr<uint8_t>(p->ws.binRecords), 0, bytes)); return BRMI_OK; }   // (bit 62: zero the records instead, so that a following frame's records can be told from older ones)
    BRMI_HIP(p, hipMemcpy(dst, p->wsPtr<uint8_t>(p->ws.binRecords), bytes, hipMemcpyDeviceToHost));
    return BRMI_OK;
}

int brmi_debug_arith(const float* a, const float* b, float* outDiv, float* outSqrt, uint32_t* outHalfBits, uint32_t n, brmi_stream stream) {
    if (!a || !b || !outDiv || !outSqrt || !outHalfBits) return BRMI_ERR_INVALID;
    if (n == 0) return BRMI_OK;
    hipLaunchKernelGGL(k_debug_arith, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a, b, outDiv, outSqrt, outHalfBits, n);
    return hipGetLastError() == hipSuccess ? BRMI_OK : BRMI_ERR_HIP;
}

int brmi_debug_arith_in_range(const float* a, float* outRcp, float* outSqrt, float* outRsqrt, uint32_t n, brmi_stream stream) {
    if (!a || !outRcp || !outSqrt || !outRsqrt) return BRMI_ERR_INVALID;
    if (n == 0) return BRMI_OK;
    hipLaunchKernelGGL(k_debug_arith_in_range, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a, outRcp, outSqrt, outRsqrt, n);
    return hipGetLastError() == hipSuccess ? BRMI_OK : BRMI_ERR_HIP;
}

int brmi_debug_ibl_lookup(const brmi_environment_buffers* env, uint32_t cubemapIndex, const float* directions, const float* lods, float* outRGBA, uint32_t n, brmi_stream stream) {
    if (!env || !environment_struct_size_ok(env->structSize) || !directions || !lods || !outRGBA) return BRMI_ERR_INVALID;
    if (n == 0u) return BRMI_OK;
    return brmi::launch_debug_ibl_lookup(environment_struct_of(env), cubemapIndex, directions, lods, outRGBA, n, static_cast<hipStream_t>(stream));
}
int brmi_debug_ibl(brmi_pass* p, const brmi_environment_buffers* env, uint32_t environmentIndex, const float* normals, const uint32_t* albedo, const uint32_t* metallicRoughness, const uint64_t* coat,
                   const uint64_t* emissive, const uint64_t* fuzz, const float* viewWS, float* outDiffuse, float* outSpecular, uint32_t n, brmi_stream stream) {
    CHECK_READY(p);
    if (!env || !environment_struct_size_ok(env->structSize) || !env->environments || environmentIndex >= env->environmentCount)
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_debug_ibl: no such environment (structSize, table or index)");
    if (!normals || !albedo || !metallicRoughness || !coat || !emissive || !fuzz || !viewWS || !outDiffuse || !outSpecular) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_debug_ibl: a null pointer");
    if (n == 0u) return BRMI_OK;
    return brmi::launch_debug_ibl(p, environment_struct_of(env), environmentIndex, normals, albedo, metallicRoughness, coat, emissive, fuzz, viewWS, outDiffuse, outSpecular, n, static_cast<hipStream_t>(stream));
}
// ---- shadow maps of spot and point lights (brmi_shadow.hip, brmi_shadow.h): every refusal comes before anything of the pass changes
int brmi_set_shadows(brmi_pass* p, const brmi_shadow_buffers* b) {
    if (!p) return BRMI_ERR_INVALID;
    if (!b) { if (p->shadows.on) p->updateSerial++; p->shadows.on = false; p->shadows.b = brmi_shadow_buffers{}; return BRMI_OK; }
    if (b->structSize != sizeof(brmi_shadow_buffers)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_shadows: structSize %u, expected %zu", b->structSize, sizeof(brmi_shadow_buffers));
    if (!p->haveScene) return brmi::fail(p, BRMI_ERR_STATE, "brmi_set_shadows: brmi_set_scene first (the binding is checked against the scene's lights and cameras)");
    if ((!b->maps && b->mapCount) || (!b->spotCameraIndices && b->spotCount) || (!b->pointCameraIndices && b->pointCount))
        return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_shadows: a null table with a non-zero count");
    if (b->pointCount > 0xFFFFFFFFu / 6u) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_shadows: pointCount %u", b->pointCount);
    // what the host can see: the lights, the descriptors and the two index arrays, read back once
    std::vector<brmi_light_info> lights; std::vector<brmi_texture_desc> maps; std::vector<uint32_t> spot, point;
    if (int rc = read_back(p, lights, p->scene.lights, p->scene.lightCount)) return rc;
    if (int rc = read_back(p, maps, b->maps, b->mapCount)) return rc;
    if (int rc = read_back(p, spot, b->spotCameraIndices, b->spotCount)) return rc;
    if (int rc = read_back(p, point, b->pointCameraIndices, (size_t)b->pointCount * 6u)) return rc;
    for (size_t i = 0; i < maps.size(); i++) {
        const brmi_texture_desc& d = maps[i];
        if (d.format != BRMI_TEXTURE_FORMAT_R32_FLOAT) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_shadows: map %zu has format %u, expected BRMI_TEXTURE_FORMAT_R32_FLOAT", i, d.format);
        if (!d.texels || d.width == 0u || d.height == 0u || d.mipCount != 1u || (reinterpret_cast<uintptr_t>(d.texels) & 3u))
            return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_shadows: map %zu needs texels (4 B aligned), a size and exactly one level", i);
    }
    for (size_t i = 0; i < spot.size(); i++) if (spot[i] >= p->scene.cameraCount) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_shadows: spot view %zu names camera %u of %u", i, spot[i], p->scene.cameraCount);
    for (size_t i = 0; i < point.size(); i++) if (point[i] >= p->scene.cameraCount) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_shadows: point view %zu names camera %u of %u", i, point[i], p->scene.cameraCount);
    for (size_t i = 0; i < lights.size(); i++) {
        const brmi_light_info& l = lights[i];
        const bool spotL = l.type == BRMI_LIGHT_SPOT, pointL = l.type == BRMI_LIGHT_POINT;
        if ((!spotL && !pointL) || l.shadowViewInfoIndex == -1 || l.shadowMapIndex == -1) continue;      // unshadowed (a directional light always is)
        const uint64_t lastMap = (uint64_t)(uint32_t)l.shadowMapIndex + (pointL ? 5u : 0u);
        if (l.shadowMapIndex < 0 || lastMap >= b->mapCount) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_shadows: light %zu names shadow map %d, the table has %u", i, l.shadowMapIndex, b->mapCount);
        if (l.shadowViewInfoIndex < 0 || (uint32_t)l.shadowViewInfoIndex >= (spotL ? b->spotCount : b->pointCount))
            return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_shadows: light %zu names %s view %d, the table has %u", i, spotL ? "spot" : "point", l.shadowViewInfoIndex, spotL ? b->spotCount : b->pointCount);
        if (pointL) for (uint32_t f = 0; f < 6u; f++) {
            const brmi_texture_desc& d = maps[(size_t)l.shadowMapIndex + f];
            if (d.width != d.height || d.width != maps[(size_t)l.shadowMapIndex].width) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_set_shadows: light %zu: the six faces from map %d on must be square and of one size", i, l.shadowMapIndex);
        }
    }
    p->shadows.b = *b; p->shadows.on = true;
    p->updateSerial++;       // the frame constants build the per-light shadow records: re-evaluated by the next stage call
    return BRMI_OK;
}
int brmi_shadow_capture(brmi_pass* p, float zNear, float zFar, const brmi_texture_desc* dst, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (!p->setupDone) return brmi::fail(p, BRMI_ERR_STATE, "brmi_shadow_capture: call brmi_setup first");
    if (!dst || !dst->texels || (reinterpret_cast<uintptr_t>(dst->texels) & 3u)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_shadow_capture: no destination (texels 4 B aligned)");
    if (dst->format != BRMI_TEXTURE_FORMAT_R32_FLOAT || dst->mipCount != 1u) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_shadow_capture: the destination must be BRMI_TEXTURE_FORMAT_R32_FLOAT with one level");
    if (dst->width != p->cfg.width || dst->height != p->cfg.height) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_shadow_capture: the destination is %u x %u, the pass renders %u x %u", dst->width, dst->height, p->cfg.width, p->cfg.height);
    if (p->stripes.count > 1u || p->bandY0 != 0u || p->bandY1 != p->cfg.height) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_shadow_capture: not with a row band or the interleaved partition (a map is a whole view)");
    if (!std::isfinite(zNear) || !std::isfinite(zFar) || !(zNear > 0.0f) || !(zFar > zNear)) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_shadow_capture: zNear %g, zFar %g", (double)zNear, (double)zFar);
    if (!p->res[BRMI_RES_LINEAR_DEPTH]) return brmi::fail(p, BRMI_ERR_STATE, "brmi_shadow_capture: the depth surface is not bound");
    return brmi::launch_shadow_capture(p, zNear, zFar, *dst, static_cast<hipStream_t>(stream));
}
int brmi_debug_shadow(brmi_pass* p, uint32_t lightIndex, const float* positionsWS, const float* normalsWS, float* outShadow, uint32_t n, brmi_stream stream) {
    if (!p) return BRMI_ERR_INVALID;
    if (!p->shadows.on) return brmi::fail(p, BRMI_ERR_STATE, "brmi_debug_shadow: no shadow maps bound (brmi_set_shadows)");
    if (lightIndex >= p->scene.lightCount) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_debug_shadow: light %u of %u", lightIndex, p->scene.lightCount);
    if (!positionsWS || !normalsWS || !outShadow) return brmi::fail(p, BRMI_ERR_INVALID, "brmi_debug_shadow: a null pointer");
    if (n == 0u) return BRMI_OK;
    return brmi::launch_debug_shadow(p, lightIndex, positionsWS, normalsWS, outShadow, n, static_cast<hipStream_t>(stream));
}
int brmi_debug_sample_grad(const brmi_scene_buffers* scene, const uint32_t* maxAnisotropy, uint32_t textureIndex, uint32_t samplerIndex, uint32_t uniformBinding, const float* uv, const float* ddx,
                           const float* ddy, float* outRGBA, uint32_t n, brmi_stream stream) {
    if (!scene || !uv || !ddx || !ddy || !outRGBA || (scene->textureCount && !scene->textures) || (scene->samplerCount && !scene->samplers)) return BRMI_ERR_INVALID;
    if (n == 0) return BRMI_OK;
    return brmi::launch_debug_sample_grad(*scene, maxAnisotropy, textureIndex, samplerIndex, uniformBinding != 0u, uv, ddx, ddy, outRGBA, n, static_cast<hipStream_t>(stream));
}

}  // extern "C"
