/*
 * brmi.h -- C ABI of libbrmi.so: the MI355X-native visibility-buffer path of BasicRenderer.
 *
 * Drop-in boundary.  In the reference this path lives behind OpenRenderGraph's pass interface
 * (`ComputePass::{DeclareResourceUsages,Setup,Update,Execute,Cleanup}`, e.g.
 * BR/include/Render/GraphExtensions/ClusterLOD/ClusterSoftwareRasterizationPass.h:16-54) and the
 * graph extension that schedules the cull/raster chain
 * (`IRenderGraphExtension`, BR/include/Render/GraphExtensions/CLodExtension.h:20-31;
 * schedule BR/src/Render/GraphExtensions/CLodExtension.cpp:1411-2095).  Those interfaces hand
 * shaders *descriptor indices*; this ABI hands kernels *device pointers* and a hipStream_t in
 * place of the command list.  One `brmi_pass` object = the CLodExtension + VisUtil + light
 * clustering + deferred shading passes of one view.  Failures are int status codes plus
 * brmi_last_error() (the reference throws; BR/src/Renderer.cpp:2112-2122); fixed-capacity
 * appends drop + count and never fault (BR/shaders/ClusterLOD/workGraphCulling.hlsl:3094-3112).
 *
 * No torch / C++ types cross this boundary: plain pointers, sizes and PODs only.
 */
#ifndef BRMI_H
#define BRMI_H

#include <stdint.h>
#include "brmi_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BRMI_ABI_VERSION 1u
/* Additions that leave every ABI-1 host binary compatible (new entry points, no changed layout) raise the minor number.  1: brmi_set_debug_view,
 * brmi_debug_view, brmi_debug_view_bytes. */
#define BRMI_ABI_MINOR 1u

typedef enum brmi_status {
    BRMI_OK            = 0,
    BRMI_ERR_INVALID   = -1,   /* bad argument / missing binding */
    BRMI_ERR_HIP       = -2,   /* a HIP call failed; see brmi_last_error() */
    BRMI_ERR_CAPACITY  = -3,   /* a declared resource is too small */
    BRMI_ERR_STATE     = -4    /* phase called out of order (e.g. execute before setup) */
} brmi_status;

typedef struct brmi_pass brmi_pass;
typedef void* brmi_stream;     /* hipStream_t; NULL = the default stream */

/* ---- configuration: the SettingsManager keys this path reads ------------------------------ */
/* defaults: BR/src/Renderer.cpp:1108-1237 ; BR/include/Renderer.h:157,216-221 */
typedef struct brmi_config {
    uint32_t structSize;               /* sizeof(brmi_config), for forward compatibility */
    uint32_t width, height;            /* visibility / G-buffer / HDR target size */
    uint32_t maxVisibleClusters;       /* CLodExtension maxClusters (Renderer.cpp:2494: 30,000,000); at most 2^25 - 1 */
    uint32_t maxTraversalRecords;      /* frontier + bucket capacity (reference shares maxClusters) */
    uint32_t enableOcclusionCulling;   /* 2-phase HZB culling (Renderer.h:157 default true) */
    uint32_t enableClusteredLighting;  /* PSO_CLUSTERED_LIGHTING (default true) */
    uint32_t enablePunctualLights;     /* DeferredShadingPass root constant (default true) */
    uint32_t lightClusterSize[3];      /* {12,12,24}  (Renderer.cpp:1154) */
    uint32_t phase2ExpansionFactor;    /* meshlets per bucket record, CLodCommon.h:31 default 2 */
    uint32_t collectPassStatistics;    /* per-stage hipEvent timing (Renderer.cpp:1133-1134) */
    uint32_t maxBvhLevels;             /* level-loop bound; reference caps at 64 (HierarchicalDispatchCullingPass.cpp:57) */
    uint32_t bandY0, bandY1;           /* rows [bandY0,bandY1) this GPU owns (multi-GPU tile split); 0,0 = all */
    uint32_t keepUniformLayerPlanes;   /* default 0 (every plane is written every frame).  1: when every material of the scene packs to the same coat
                                          (fuzz) G-buffer word and binds no coat / fuzz texture, the plane is filled with that word once after brmi_setup
                                          and brmi_execute skips the per-frame stores to it (16 of 52 B per pixel).  Only for hosts that neither write,
                                          clear nor alias GBUF_COAT / GBUF_FUZZ between frames. */
    /* Interleaved screen partition, round 3.  stripeCount > 1: a frame `fullHeight` rows high is cut into chunks of `stripeRows`
     * rows (a multiple of 16), stripeCount consecutive chunks form a group, and this GPU owns one chunk of every group -- chunk stripeIndex of
     * the even groups, chunk stripeCount - 1 - stripeIndex of the odd ones (back and forth, so that a vertical cost gradient does not favour
     * one GPU) -- and renders them into COMPACT surfaces: `height` is then the number of rows it owns (fullHeight / stripeCount; fullHeight a
     * multiple of stripeRows * stripeCount), and row v of every surface is row (g * stripeCount + slot(g)) * stripeRows + v % stripeRows of the
     * frame, g = v / stripeRows.  Cameras, lights and perFrame.screenResY describe the FULL frame.  bandY0 / bandY1 stay 0.
     * 0 / 1: off (the contiguous band of bandY0 / bandY1, or the whole frame). */
    uint32_t stripeRows, stripeCount, stripeIndex, fullHeight;
    /* Round 6: 1 = the band may change from frame to frame (brmi_set_band; cost-balanced contiguous regions): per-band workspace tables are sized for
     * the whole frame.  bandY0 / bandY1 are then the first frame's band.  Not with the interleaved partition. */
    uint32_t dynamicBand;
    uint32_t reserved[2];
} brmi_config;

void brmi_default_config(brmi_config* cfg, uint32_t width, uint32_t height);

/* ---- scene providers (IResourceProvider keys, BR/include/Renderer.h:284-323) ----------------
 * Device pointers to the structured buffers the reference's managers own.  `slabs` is a device
 * array of device pointers indexed by slabDescriptorIndex (entry 0 unused = "not resident").   */
typedef struct brmi_scene_buffers {
    const uint8_t* const*                  slabs;            uint32_t slabCount;        /* incl. entry 0 */
    const brmi_per_object*                 perObject;        uint32_t perObjectCount;
    const float*                           normalMatrices;   /* float[4][4] per object */
    const brmi_per_mesh*                   perMesh;          uint32_t perMeshCount;
    const brmi_per_mesh_instance*          perMeshInstance;  uint32_t perMeshInstanceCount;
    const brmi_mesh_instance_clod_offsets* clodOffsets;
    const brmi_clod_mesh_metadata*         meshMetadata;     uint32_t meshMetadataCount;
    const brmi_lod_node*                   lodNodes;         uint32_t lodNodeCount;     /* nodes, groups and segments are topology: brmi_set_scene folds them into derived tables; call it again when they change */
    const brmi_lod_group*                  lodGroups;        uint32_t lodGroupCount;
    const brmi_lod_segment*                lodSegments;      uint32_t lodSegmentCount;
    const brmi_group_page_map_entry*       groupPageMap;     uint32_t groupPageMapCount;
    const brmi_material_info*              materials;        uint32_t materialCount;
    const brmi_openpbr_material_info*      openpbrMaterials; uint32_t openpbrMaterialCount;   /* at most 65536: the shading pass keeps 66 KB of folded table rows per record in the workspace (brmi_set_scene refuses more) */
    const brmi_light_info*                 lights;           uint32_t lightCount;
    const uint32_t*                        activeLightIndices;
    const brmi_camera*                     cameras;          uint32_t cameraCount;
    const brmi_culling_camera*             cullingCameras;
    const brmi_view_raster_info*           viewRasterInfo;
    const brmi_per_frame*                  perFrame;
    const uint32_t*                        activeDraws;      uint32_t activeDrawCount;  /* per-mesh-instance indices */
    const float*                           skinningMatrices; uint32_t skinningMatrixCount; /* float[4][4]: bone*invBind */
    /* OpenPBR lookup tables (BR/src/Render/OpenPBRLookupResources.cpp:34-77): R16_UNORM energy
     * tables 32x32(x32) and the 32x32 float LTC table, injected by the caller. */
    const uint16_t* lutOpaqueDielectricEnergyComplement;     /* [32 ior][32 alpha][32 cos] */
    const uint16_t* lutOpaqueDielectricAvgEnergyComplement;  /* [32 ior][32 alpha] */
    const uint16_t* lutIdealMetalEnergyComplement;           /* [32 alpha][32 cos] */
    const uint16_t* lutIdealMetalAvgEnergyComplement;        /* [32 alpha] */
    const float*    lutFuzzLTC;                               /* [32 rough][32 cos][4]: aInv,bInv,refl,0 */
    /* material textures (the descriptor-heap slots MaterialInfo indexes); all may be null / 0 for a scene of
     * constant-factor materials.  srgbToLinear: float[256], the sRGB decode of an 8-bit code (injected like the LUTs:
     * pow() differs between math libraries). */
    const brmi_texture_desc* textures;     uint32_t textureCount;
    const brmi_sampler_desc* samplers;     uint32_t samplerCount;
    const float*             srgbToLinear;
} brmi_scene_buffers;

/* ---- residency and streaming feedback (CLodStreaming*; optional) ------------------------------
 * With these bound the cluster-LOD cut follows the reference's full rule "... and the refined child group is resident" (workGraphCulling.hlsl:1543-1701,
 * 1713-1783): a leaf whose own group is not resident is not drawn, a parent whose refined child is not resident keeps drawing, and the culling
 * kernels record which groups the frame touched and which it wants loaded.  All of it is caller-owned device memory (the library never allocates);
 * passes that render frames in turn bind their own.
 *   loadRequests   one record per REQUESTED GROUP (not per requesting thread, as the reference's raw stream has it): the highest priority any request
 *                  of the frame gave the group, among the requests of that priority the lowest instance index and that instance's perMeshBufferIndex;
 *                  ordered by descending priority, then ascending group index.  More than requestCapacity: the first requestCapacity of that order.
 *   touchedGroups  the touched group indices in ascending order, under the same truncation rule.
 *   counts         [0] = requested groups, [1] = touched groups of the frame, whatever the capacities.
 * This is what the reference's host makes of its stream after read-back (CLodStreamingSystem::PushOrUpdatePendingStreamingRequest). */
typedef struct brmi_streaming_buffers {
    uint32_t structSize;                     /* sizeof(brmi_streaming_buffers) */
    uint32_t activeGroupScanCount;           /* CLodStreamingRuntimeState: groups at or above it are non-resident and are never requested (clamped to lodGroupCount) */
    const uint32_t* nonResidentBits;         /* Builtin::CLod::StreamingNonResidentBits: bit g set = group g (index into lodGroups) is not resident; ceil(lodGroupCount / 32) words */
    brmi_streaming_request* loadRequests;    uint32_t requestCapacity;   /* Builtin::CLod::StreamingLoadRequests (reference: 1 << 16) */
    uint32_t* touchedGroups;                 uint32_t touchedCapacity;   /* Builtin::CLod::StreamingTouchedGroups (reference: 1 << 17) */
    uint32_t* counts;                        /* two words: StreamingLoadCounter, StreamingTouchedGroupsCounter */
    void* scratch;                           uint64_t scratchBytes;      /* >= brmi_streaming_scratch_bytes(lodGroupCount), 16 B aligned; the library's between the frame's first culling launch and brmi_streaming_feedback */
} brmi_streaming_buffers;

/* ---- debug views: perFrame.outputType (BR/shaders/Include/outputTypes.hlsli) ------------------
 * The modes this path builds.  The payload is the reference's (Include/debugPayload.hlsli): one uint2 per pixel, (0xFFFFFFFF, 0xFFFFFFFF) where the
 * pixel has no geometry; float3 modes hold three RNE halves in x low, x high, y low, integer modes hold (v, 0).  The material modes (ALBEDO, METALLIC,
 * ROUGHNESS, AO, MOTION_VECTORS) pack what the G-buffer planes HOLD, i.e. the value after the plane's format quantised it; the reference packs the
 * material inputs before that.  Every other outputType (MODEL_NORMALS, SW_RASTER, MATERIAL_SELECTED_MIP, the IBL / VSM / Reyes /
 * voxel / transparency modes) is refused by brmi_debug_view. */
typedef enum brmi_output_type {
    BRMI_OUTPUT_COLOR = 0,                        /* the lit frame: no debug payload */
    BRMI_OUTPUT_NORMAL = 1,                       /* normals.xyz * 0.5 + 0.5 */
    BRMI_OUTPUT_ALBEDO = 2,
    BRMI_OUTPUT_METALLIC = 3,
    BRMI_OUTPUT_ROUGHNESS = 4,
    BRMI_OUTPUT_EMISSIVE = 5,
    BRMI_OUTPUT_AO = 6,                           /* albedo.a; with brmi_set_gtao bound, min(albedo.a, aoTerm / 255) (deferred.hlsl:70-71) */
    BRMI_OUTPUT_DEPTH = 7,                        /* |linear depth| * 0.1 */
    BRMI_OUTPUT_MESHLETS = 10,                    /* page-local meshlet index of the pixel's visible cluster */
    BRMI_OUTPUT_LIGHT_CLUSTER_ID = 12,            /* the light cluster's depth slice (lighting.hlsli:509), at most lightClusterSize[2] */
    BRMI_OUTPUT_LIGHT_CLUSTER_LIGHT_COUNT = 13,   /* numLights of the pixel's light cluster; needs enableClusteredLighting */
    BRMI_OUTPUT_MOTION_VECTORS = 14,              /* (mv * 0.5 + 0.5, 0.5) */
    BRMI_OUTPUT_GEOMETRY_GROUP = 35               /* LOD group id of the pixel's visible cluster */
} brmi_output_type;

/* Caller-owned device memory of the debug view (never part of brmi_declare's list).  payload: one uint2 per pixel in the surfaces' tiled 8x8 layout,
 * brmi_debug_view_bytes(width, height) bytes (whole tiles), 16 B aligned; the library writes every pixel of the band, the sentinel included.  image:
 * optional (NULL = payload only) rgba8, ROW-MAJOR width x height x 4 bytes -- the one surface meant to be looked at; pixels whose payload is the sentinel
 * are NOT written (the reference's resolve discards them), so what the caller put there shows through. */
typedef struct brmi_debug_view_buffers {
    uint32_t structSize;              /* sizeof(brmi_debug_view_buffers) */
    uint32_t reserved;
    void*    payload;  uint64_t payloadBytes;
    void*    image;    uint64_t imageBytes;      /* >= width * height * 4 when image is bound */
} brmi_debug_view_buffers;

/* ---- graph resources the pass declares (DeclareResourceUsages) ---------------------------- */
typedef enum brmi_resource_id {
    BRMI_RES_VISIBILITY = 0,          /* Builtin::PrimaryCamera::VisibilityTexture  u64/px, tiled 8x8 */
    BRMI_RES_LINEAR_DEPTH,            /* Builtin::PrimaryCamera::LinearDepthMap     f32/px, tiled */
    BRMI_RES_GBUF_NORMALS,            /* Builtin::GBuffer::Normals            float4  */
    BRMI_RES_GBUF_ALBEDO,             /* Builtin::GBuffer::Albedo             rgba8 unorm */
    BRMI_RES_GBUF_COAT,               /* Builtin::GBuffer::Coat               rgba16f */
    BRMI_RES_GBUF_EMISSIVE,           /* Builtin::GBuffer::Emissive           rgba16f */
    BRMI_RES_GBUF_FUZZ,               /* Builtin::GBuffer::Fuzz               rgba16f */
    BRMI_RES_GBUF_METALLIC_ROUGHNESS, /* Builtin::GBuffer::MetallicRoughness  rgba8 unorm */
    BRMI_RES_GBUF_MOTION_VECTORS,     /* Builtin::GBuffer::MotionVectors      rg16f */
    BRMI_RES_HDR_COLOR,               /* Builtin::Color::HDRColorTarget       rgba16f; like the G-buffer planes, pixels without geometry are NOT
                                         written (DeferredCSMain returns, BR/shaders/deferred.hlsl:33-37): the graph clears / the sky pass fills them */
    BRMI_RES_VISIBLE_CLUSTERS,        /* CLod visible-cluster buffer, 16 B records */
    BRMI_RES_LIGHT_CLUSTERS,          /* Builtin::Light::ClusterBuffer */
    BRMI_RES_LIGHT_PAGES,             /* Builtin::Light::PagesBuffer */
    BRMI_RES_HZB,                     /* linear-depth mip chain for occlusion culling */
    BRMI_RES_WORKSPACE,               /* frontiers, bucket records, bitmasks, counters, statistics */
    BRMI_RES_COUNT
} brmi_resource_id;

typedef enum brmi_usage {
    BRMI_USAGE_SHADER_RESOURCE  = 1u << 0,
    BRMI_USAGE_UNORDERED_ACCESS = 1u << 1,
    BRMI_USAGE_INTERNAL         = 1u << 2     /* no consumer outside this pass; may be aliased */
} brmi_usage;

typedef struct brmi_resource_desc {
    uint32_t    id;             /* brmi_resource_id */
    const char* name;           /* the reference's Builtin:: key this resource stands for */
    uint64_t    bytes;          /* required size */
    uint32_t    usage;          /* brmi_usage mask */
    uint32_t    width, height;  /* logical size in pixels (0 for buffers) */
    uint32_t    bytesPerPixel;
    uint32_t    tileW, tileH;   /* storage tiling (8x8, column-major inside a tile); pixel (x,y) lives at
                                   ((y/tileH)*tilesX + x/tileW)*tileW*tileH + (x%tileW)*tileH + y%tileH */
} brmi_resource_desc;

typedef void (*brmi_declare_cb)(void* user, const brmi_resource_desc* desc);

typedef struct brmi_resource_binding { uint32_t id; void* ptr; uint64_t bytes; } brmi_resource_binding;

/* per-frame host data (UpdateExecutionContext) */
typedef struct brmi_frame_update {
    const brmi_camera*    mainCameraHost;   /* host copy of cameras[perFrame.mainCameraIndex] */
    const brmi_per_frame* perFrameHost;     /* host copy of the per-frame constant buffer */
    uint32_t              frameIndex;
} brmi_frame_update;

/* counters read back after a frame (the reference's GPU telemetry, CLodTelemetry.h) */
typedef struct brmi_counters {
    uint32_t instancesTested, instancesVisible;
    uint32_t nodesVisited, bucketRecords;
    uint32_t meshletsTested, visibleClusters, visibleClustersPhase2;
    uint32_t droppedRecords, droppedClusters;
    uint32_t lightPagesUsed;
    uint32_t replayNodes, replayMeshlets;   /* occluded in phase 1, re-tested in phase 2 */
    /* Statistics of the rasteriser (no counterpart in CLodTelemetry.h).  [0] / [2]: vertex / triangle count sums of the visible clusters, both phases (32 bits
     * each since round 5: brmi_create refuses a cluster capacity whose sums could exceed them).  [4]: clusters handed to the rasteriser stage; [5]: raster records
     * that found their screen bin full.  Round 6, the draw list: [1] = clusters of the phase-1 visible list the culling HELD BACK as probably
     * hidden, [3] = how many of those the re-test could not prove hidden and the late pass drew; [1] - [3] clusters of the list were never rasterised, and the
     * image is the one of rasterising all of them.  Both 0 on frames that draw the list in order (no previous depth chain, multi-GPU partitions, hold_clusters=0). */
    uint32_t reserved[6];
} brmi_counters;

enum brmi_stage {
    BRMI_STAGE_CLEAR = 0, BRMI_STAGE_CULL, BRMI_STAGE_RASTER, BRMI_STAGE_DEPTH_COPY, BRMI_STAGE_HZB,
    BRMI_STAGE_CULL2, BRMI_STAGE_RASTER2, BRMI_STAGE_GBUFFER, BRMI_STAGE_LIGHT_CLUSTER, BRMI_STAGE_SHADE,
    BRMI_STAGE_COUNT
};

/* ---- lifecycle (ComputePass phases) -------------------------------------------------------- */
uint32_t    brmi_abi_version(void);
uint32_t    brmi_abi_minor(void);
int         brmi_create(const brmi_config* cfg, brmi_pass** out);
int         brmi_declare(brmi_pass* pass, brmi_declare_cb cb, void* user);            /* DeclareResourceUsages */
int         brmi_set_scene(brmi_pass* pass, const brmi_scene_buffers* scene);          /* provider resolution   */
/* Setup also reads the resident pages once (round 6): the object-space box of every meshlet goes into a side table of the workspace (the draw list's tests, DESIGN.md 4.3c;
 * brmi_set_scene walked the page map for the table's size).  A host that rewrites page CONTENTS afterwards (streaming) calls brmi_set_scene + brmi_setup again; with
 * BRMI_TUNING=hold_clusters=0 the table is neither sized nor made. */
int         brmi_setup(brmi_pass* pass, const brmi_resource_binding* b, uint32_t n, brmi_stream stream); /* Setup */
int         brmi_update(brmi_pass* pass, const brmi_frame_update* upd, brmi_stream stream);               /* Update */
int         brmi_execute(brmi_pass* pass, brmi_stream stream);                          /* Execute: whole chain */
/* The same frame on two streams (the reference's graph owns a graphics, a compute and a copy queue and passes state a preference: `QueueKind`, `PreferQueue`; DeviceManager.cpp:178): culling, rasterisation
 * and the depth chain on `geometryStream`, G-buffer, light lists (when the culling launches did not carry them) and shading on
 * `shadingStream`; events order the two halves and the pass's next frame.  Outputs are ready when `shadingStream` is.  With
 * brmi_set_history_source and two passes alternating frames on the same geometry stream (the shading stream may be shared or one per
 * pass), frame k+1's geometry half -- latency-bound launches that leave most of the chip idle -- runs beside frame k's shading half;
 * give `geometryStream` the higher priority.
 * Per-frame inputs with frames in flight: the resolve + shading half reads the camera and the per-frame record from a copy the frame's
 * first launch makes in the pass's workspace, so the caller may rewrite `cameras`, `cullingCameras`, `viewRasterInfo` and `perFrame` for the
 * pass's NEXT frame as soon as this call has returned -- ON `geometryStream`, before the brmi_update of that frame (stream order then puts
 * the write behind this frame's geometry half and in front of the next frame's).  Passes that render frames in turn must not share these
 * buffers (each pass binds its own: brmi_set_scene), and buffers every frame reads but none owns (lights, materials, objects, geometry)
 * may only change while no frame that reads them is in flight.
 * The stage entry points that start a frame (brmi_clear_visibility, brmi_cull(1)) issue the same waits as this call, so a graph that runs
 * the stages itself after a split frame is ordered behind that frame's shading half. */
int         brmi_execute_split(brmi_pass* pass, brmi_stream geometryStream, brmi_stream shadingStream);
void        brmi_destroy(brmi_pass* pass);                                               /* Cleanup */
const char* brmi_last_error(const brmi_pass* pass);

/* Residency-aware cut + streaming feedback.  Call after brmi_set_scene (which forgets the binding: the group table may have changed); NULL switches it off
 * and gives exactly the frames of a pass that never called it.  Refuses (BRMI_ERR_INVALID / BRMI_ERR_CAPACITY) a null required pointer or scratch that is
 * too small.  The residency bits are read by the frame's culling launches: rewrite them between frames, in stream order with the frames. */
uint64_t brmi_streaming_scratch_bytes(uint32_t lodGroupCount);
int brmi_set_streaming(brmi_pass* pass, const brmi_streaming_buffers* streaming);

/* Per-sampler maxAnisotropy for the G-buffer pass's SampleGrad (up to maxAnisotropy SampleLevel taps along the footprint's major axis; a word is
 * clamped to [1, 16], 0 reads as 1; the parallax march's height fetches and the rasteriser's alpha test stay isotropic).  `maxAnisotropy`: DEVICE pointer to
 * samplerCount words, caller-owned, read by the frame's G-buffer launch.  NULL switches it off and gives exactly the frames of a pass that never called it.
 * Call after brmi_set_scene (which forgets the binding).  BRMI_ERR_INVALID: count != the scene's samplerCount. */
int brmi_set_sampler_anisotropy(brmi_pass* pass, const uint32_t* maxAnisotropy, uint32_t count);

/* Image-based lighting: with an environment bound the shading pass adds evaluateIBL (BR/shaders/Include/IBL.hlsli:683-740) as the first addend of
 * a pixel's lighting, in fp32 inside the shading kernel, as lightFragment does under PSO_IMAGE_BASED_LIGHTING.  The environment of a frame is
 * perFrameHost->activeEnvironmentIndex of that frame's brmi_update.  prefilteredCubemapDescriptorIndex indexes `cubemaps` in whole cubemaps; a TextureCube's
 * SampleLevel(g_linearClamp, dir, lod) is the software definition of DESIGN.md 2 (major axis, the 2D sampler on that face, no filtering across face edges).
 * All memory is caller-owned DEVICE memory that every frame reads and none owns (the rule of brmi_execute_split for lights and materials).
 * NULL switches it off and gives exactly the frames -- kernels, bytes -- of a pass that never called it.  brmi_set_scene does NOT forget this binding: nothing of
 * it depends on the scene.
 * Refused with BRMI_ERR_INVALID before anything is launched: a wrong structSize, a null table with a non-zero count, environmentCount == 0, and (here and at
 * brmi_update) an activeEnvironmentIndex >= environmentCount.  What the host cannot see is the caller's contract: the six faces of a cubemap are square, of one
 * size, mipCount and BRMI_TEXTURE_FORMAT_RGBA8_UNORM, every chain inside its allocation.  The kernel reads each face by that face's own descriptor, clamps texel
 * coordinates and levels to it, and reads a cubemap index >= cubemapCount or a descriptor without texels, size or levels (or with more than
 * BRMI_TEXTURE_MAX_MIPS) as zero radiance: it never faults on a table that disagrees with itself.
 * The PREFILTERED cube stays RGBA8 (the reference's R8G8B8A8_UNorm; brmi_env_prefilter writes that): the shading pass takes every face of it as
 * BRMI_TEXTURE_FORMAT_RGBA8_UNORM.  Only the cube cubeMapDescriptorIndex names -- the one the skybox stage shows -- may be BRMI_TEXTURE_FORMAT_RGBA16_FLOAT.
 * `skybox` (the reference's SkyboxRenderPass, Deferred -> Skybox -> Forward): with it set, brmi_execute / brmi_execute_split run brmi_skybox behind the shading
 * stage on the shading stream, in front of the debug-view stage; without it a frame launches exactly what it launched before the field existed.  structSize
 * says whether the field is there: a struct of the size before it (BRMI_ENVIRONMENT_BUFFERS_SIZE_V1) is accepted and means `skybox` = 0. */
typedef struct brmi_environment_buffers {
    uint32_t structSize;
    uint32_t specularIBL;                        /* PSO_SPECULAR_IBL: the reference defines it whenever screen-space reflections are off (PSOManager.cpp:1908-1913) */
    const brmi_environment_info* environments;   uint32_t environmentCount;   /* Builtin::Environment::InfoBuffer, device */
    uint32_t reserved0;                          /* (the padding of the first layout: not read) */
    const brmi_texture_desc*     cubemaps;       uint32_t cubemapCount;       /* device; cubemap c = entries 6c .. 6c+5 in the order +X -X +Y -Y +Z -Z */
    uint32_t reserved1;                          /* (the padding of the first layout: not read) */
    uint32_t skybox;                             /* 0 / 1; read only when structSize covers it */
    uint32_t reserved2[3];                       /* room for the next switches, zero for now.  (They also keep sizeof - 8 from being the first layout's size,
                                                    which stays an accepted structSize: a struct that has lost its last fields must not pass for the old one.) */
} brmi_environment_buffers;                      /* 56 B */
#define BRMI_ENVIRONMENT_BUFFERS_SIZE_V1 40u     /* the struct up to and including cubemapCount's padding */
int brmi_set_environment(brmi_pass* pass, const brmi_environment_buffers* env);
/* SkyboxRenderPass (BR/shaders/skybox.hlsl): every pixel of the band whose linear depth is "empty" (0x7F7FFFFF) gets the lod-0 lookup of cubemap
 * cubeMapDescriptorIndex of the frame's environment (RGBA16F or RGBA8) along its view ray as half4(colour, 1) in the lit HDR target, and currentNdc - prevNdc of
 * that direction in the motion-vector plane (rg16f); pixels with geometry are not touched.  One wave per 8x8 tile of the surfaces' layout; a tile without an
 * empty pixel ends before it loads the camera.  IEEE fp32 without contraction, normalize = v * (1 / sqrt(dot(v, v))) with both correctly rounded.
 * Row bands write their rows only; the interleaved partition works as in the shading pass (the row table of the compact surfaces names the frame's rows).
 * BRMI_ERR_STATE before brmi_setup / brmi_update, or without a bound environment whose `skybox` is set. */
int brmi_skybox(brmi_pass* pass, brmi_stream stream);

/* ---- environment build: the reference's EnvironmentConversionPass, EnvironmentSHPass and EnvironmentFilterPass ---------------------------
 * Three stages on caller-owned DEVICE memory; they need no pass.  Every descriptor table is a device pointer; a cube is six brmi_texture_desc in the order
 * +X -X +Y -Y +Z -Z.  Each kernel reads and writes every face through that face's own descriptor, clamps to it, and skips a face whose descriptor has no texels,
 * size or levels, or not the format the stage writes: it never faults on a table that disagrees with itself (chains inside their allocations are the caller's
 * contract, as for brmi_set_environment).  Lookups of the source are SampleLevel(g_linearClamp, .., 0) by the definition of DESIGN.md 2 (the reference's source cube
 * has one level), RGBA16F or RGBA8.
 * Refused with BRMI_ERR_INVALID before any launch: a null table, size == 0 or > 16384, levels == 0 or > BRMI_TEXTURE_MAX_MIPS, a destination format other than the
 * one the stage writes (convert: RGBA16_FLOAT, prefilter: RGBA8_UNORM), environmentIndex >= environmentCount.
 *
 * brmi_env_convert     envToCubemap.hlsl: the equirectangular `equirect` (one descriptor, level 0) to the six faces of `cube`, size x size, alpha 1.
 * brmi_env_project_sh  sphericalHarmonics.hlsl: the 27 integers of environments[environmentIndex] from cubemap cubeMapDescriptorIndex of that record (size = its
 *                      face size, the reference's root constant); the 27 words are zeroed first and sphericalHarmonicsScale = 4 pi / (size^2 * 6) is written.
 *                      Integer sums, added as unsigned: the result does not depend on the order and wraps where the reference's InterlockedAdd wraps.
 * brmi_env_prefilter   blurEnvironment.hlsl + EnvironmentFilterPass.h:99-127: level m of `prefiltered` (size_m = max(1, size >> m)) with roughness m / (levels - 1)
 *                      (0 for one level), 16 GGX samples, RGBA8 UNORM (saturate, round to nearest), alpha 255.
 * brmi_env_build_bytes bytes of the RGBA16F cube (*cubeBytes) and of the RGBA8 chain of `levels` levels (*prefilteredBytes), six faces each, tightly packed;
 *                      returns their sum (0 for a refused size / levels).  Either pointer may be null. */
int brmi_env_convert(const brmi_texture_desc* equirect, const brmi_texture_desc* cube, uint32_t size, uint32_t cubeFormat, brmi_stream stream);
int brmi_env_project_sh(const brmi_texture_desc* cubemaps, uint32_t cubemapCount, brmi_environment_info* environments, uint32_t environmentCount,
                        uint32_t environmentIndex, uint32_t size, brmi_stream stream);
int brmi_env_prefilter(const brmi_texture_desc* sourceCube, const brmi_texture_desc* prefiltered, uint32_t size, uint32_t levels, uint32_t prefilteredFormat,
                       brmi_stream stream);
uint64_t brmi_env_build_bytes(uint32_t size, uint32_t levels, uint64_t* cubeBytes, uint64_t* prefilteredBytes);

/* ---- texture mip chains: the reference's MipmappingPass -- mipmapping.hlsl over ffx_spd.h, alphaCoverageMipmapping.hlsl ---------------------
 * Two stages on caller-owned DEVICE memory; they need no pass and allocate nothing.  `texture` is ONE descriptor in HOST memory, read during the call (the
 * refusals below need its fields); its `texels` is a device pointer to the whole packed chain (brmi_types.h: level l is max(1, w >> l) x max(1, h >> l) RGBA8
 * texels, mipOffset[l] texels after `texels`) with level 0 filled.  Levels 1 .. mipCount - 1 are written, every texel of them; level 0 and everything outside the
 * levels are not touched.  mipCount == 1 launches nothing.  `srgbToLinear`: the scene's float[256] decode table (device); with BRMI_TEXTURE_FORMAT_RGBA8_UNORM_SRGB
 * level 0's rgb is decoded through it and every stored level is encoded with LinearToSrgb of the shader text.
 *
 * brmi_texmips_build        the plain chain (SPD's Float4 variant), one launch.  `scratch`: brmi_texmips_bytes' scratchBytes, ZERO before the first build;
 *                           the build leaves it zero, so it serves every later build on the same stream without a clear.  Width and height <= 4096.
 * brmi_texmips_build_alpha  the alpha-coverage chain: per level reset, downsample + statistics, scale, apply.  `stats` (260 words per level: covered and total
 *                           count of the source level, destination count, 256-bin histogram, one pad) and `scales` (one float per level) are outputs the
 *                           caller may read; the words of level 0 are not written.
 * brmi_texmips_bytes        the three sizes for a chain of mipCount levels; returns their sum (0 for a refused mipCount).  Any pointer may be null.
 *
 * The alpha chain has no size limit of its own, and `stats` / `scales` come without byte counts: the caller is trusted to have sized them with
 * brmi_texmips_bytes, as it is trusted with the chain's own allocation.
 * Refused before any launch, with the reason in brmi_last_error(NULL): a null pass reads the calling thread's last stage refusal ("null pass" when there is
 * none; a stage call that succeeds clears it): BRMI_ERR_INVALID for a null or misaligned (4 B) pointer, a format
 * other than the two RGBA8 ones, an empty image, mipCount 0 or above BRMI_TEXTURE_MAX_MIPS or longer than the size allows, levels that overlap;
 * BRMI_ERR_CAPACITY for scratch that is too small or (plain chain) an image beyond 4096 texels. */
uint64_t brmi_texmips_bytes(uint32_t mipCount, uint64_t* scratchBytes, uint64_t* statsBytes, uint64_t* scalesBytes);
int brmi_texmips_build(const brmi_texture_desc* texture, const float* srgbToLinear, void* scratch, uint64_t scratchBytes, brmi_stream stream);
int brmi_texmips_build_alpha(const brmi_texture_desc* texture, const float* srgbToLinear, uint32_t* stats, float* scales, brmi_stream stream);

/* ---- XeGTAO ambient occlusion: the reference's BuildGTAOPipeline -- GTAOFilterPass, GTAOMainPass, GTAODenoisePass -----------------------
 * Off by default: a pass that never calls brmi_set_gtao, or calls it with NULL, launches exactly what it launched before and writes the same bytes.  With it
 * bound, brmi_execute / brmi_execute_split run the three stages between the G-buffer stage and the shading stage (on the shading stream, inside the shading
 * stage's event pair), whether or not an environment is bound; the shading pass's environment term (k_shade_ibl) then takes
 * diffuseAmbientOcclusion = min(albedo.a, aoTerm / 255) (utilities.hlsli:2663-2671) and BRMI_OUTPUT_AO packs that minimum.  Punctual lights never read it.
 * brmi_shade on its own runs no GTAO stage: it reads the term the last brmi_gtao_denoise left.
 * Every plane is in the surfaces' tiled 8x8 layout (brmi_resource_desc's formula) at its own size, in whole tiles.  All of it is caller-owned DEVICE memory,
 * never part of brmi_declare's list (like the debug view's targets); brmi_set_scene does not forget the binding.
 * qualityLevel 0..3 = Low (1 slice x 2 steps), Medium (2 x 2), High (3 x 3: what the reference dispatches, the default), Ultra (9 x 3).
 * denoisePasses 0..3: 0 = one pass with blur beta 1e4 (the reference's "disabled"); 1 = one final pass, beta 1.2; n > 1 = n - 1 passes with beta / 5 that
 * ping-pong between the two working terms, then the final one.
 * maxDepthLod 0..4: the highest depth level a tap may read.  0 is the reference as written (its sampler's maxLod = 0 clamps SampleLevel), 4 is XeGTAO as its
 * authors meant it; the prefilter writes all five levels either way.
 * The temporal index of the noise is frameIndex % 64 of the frame's brmi_update; the constants (GTAOUpdateConstants) are made on the host from the main
 * camera's fov and aspectRatio of that update and the frame size.
 * brmi_set_gtao refuses with BRMI_ERR_INVALID, before anything is launched: a wrong structSize (of the buffers or the settings), a null, misaligned (16 B) or
 * short scratch / aoTerm, qualityLevel > 3, denoisePasses > 3, a radius that is not finite or <= 0, maxDepthLod > 4, and A PASS WITH A ROW BAND, dynamicBand OR
 * STRIPES: the taps of a pixel reach up to the effect radius in every direction, into rows another GPU owns and this one never rendered. */
typedef struct brmi_gtao_settings {
    uint32_t structSize;        /* sizeof(brmi_gtao_settings) */
    uint32_t qualityLevel;      /* 0..3, default 2 */
    uint32_t denoisePasses;     /* 0..3, default 1 */
    float    radius;            /* view-space effect radius, default 0.5 */
    uint32_t maxDepthLod;       /* 0..4, default 0 */
    uint32_t reserved[3];       /* zero */
} brmi_gtao_settings;           /* 32 B */
typedef struct brmi_gtao_plane { uint64_t offset; uint32_t width, height; } brmi_gtao_plane;      /* byte offset into the scratch, size in pixels */
typedef struct brmi_gtao_layout {
    brmi_gtao_plane depth[5];   /* R32F: level m is max((size + 2^m - 1) >> m, 1) pixels */
    brmi_gtao_plane edges;      /* R8: the packed edges of the main pass */
    brmi_gtao_plane term[2];    /* R8: the working terms (the main pass writes [0]) */
    uint64_t scratchBytes;      /* what brmi_gtao_buffers::scratch must hold */
    uint64_t outputBytes;       /* what brmi_gtao_buffers::aoTerm must hold: 1 B per pixel, tiled, whole tiles */
} brmi_gtao_layout;             /* 144 B */
typedef struct brmi_gtao_buffers {
    uint32_t structSize;        /* sizeof(brmi_gtao_buffers) */
    uint32_t reserved;
    brmi_gtao_settings settings;
    void*    scratch;  uint64_t scratchBytes;
    void*    aoTerm;   uint64_t aoTermBytes;      /* the final term: visibility code per pixel, 255 = unoccluded */
} brmi_gtao_buffers;            /* 72 B */
void brmi_gtao_default_settings(brmi_gtao_settings* settings);
int  brmi_gtao_get_layout(uint32_t width, uint32_t height, brmi_gtao_layout* layout);      /* BRMI_ERR_INVALID: a null layout or an empty frame */
int  brmi_set_gtao(brmi_pass* pass, const brmi_gtao_buffers* buffers_or_NULL);
/* The stages.  BRMI_ERR_STATE before brmi_setup / brmi_update, or when nothing is bound.  prefilter: the linear-depth surface -> the five depth levels;
 * main: levels + the normals plane -> edges and working term [0]; denoise: edges + working term -> aoTerm (through the second working term for
 * denoisePasses > 1). */
int  brmi_gtao_prefilter(brmi_pass* pass, brmi_stream stream);
int  brmi_gtao_main(brmi_pass* pass, brmi_stream stream);
int  brmi_gtao_denoise(brmi_pass* pass, brmi_stream stream);

/* ---- The display chain: the reference's LuminanceHistogramPass, LuminanceHistogramAveragePass, BuildBloomPipeline and TonemappingPass --------
 * Off by default: a pass that never calls brmi_set_display, or calls it with NULL, launches exactly what it launched before and writes the same bytes.  With it
 * bound, brmi_execute / brmi_execute_split run brmi_display_exposure, brmi_display_bloom and brmi_display_resolve behind the skybox stage, on the shading stream,
 * inside the shading half's ordering: `ldr` is ready when the shading stream is.  The pass's HDR target is only read.
 *
 * tonemapType        0 Reinhard-Jodie, 1 Khronos PBR Neutral, 2 ACES (Hill), 3 AMD LPM (the default, as the reference's `tonemapType` setting), 4 none (gamma only)
 * bloom              1: five downsamples (level l is (W >> l) x (H >> l), l = 1 .. min(5, floor(log2(max(W, H))) + 1)), the additive tent upsamples and the 0.04
 *                    blend, which brmi_display_resolve applies on the way (blendedHdr, when given, receives the blended level 0).  Refused below 32 pixels a side.
 * autoExposure       1: the 256-bin histogram and its average drive the adapted luminance, adapted += (average - adapted) * timeCoefficient (the reference passes
 *                    the frame's delta time, unclamped), and the LPM control block follows it.  0: no histogram stage; fixedAdaptedLuminance feeds the block.
 * minLogLuminance, logLuminanceRange   the histogram's range (defaults 0.001 and log2(10) - log2(0.1), the reference's).
 * All memory is the caller's, none of it part of brmi_declare: `scratch` (brmi_display_get_layout: the histogram, the adapted-luminance float, the 96-word LPM
 * control block, the bloom levels in the surfaces' tiled layout, whole tiles), `ldr` (row-major R8G8B8A8, W * H * 4 bytes), `blendedHdr` (optional, tiled
 * RGBA16F).  The caller zeroes the histogram and the adapted luminance ONCE: the average stage leaves the histogram zero, and the adapted luminance is the only
 * state carried from frame to frame.  Passes that render frames in turn may share one scratch only if their shading streams are the same stream.
 * brmi_set_display is host-only and cheap: call it between frames with the same buffers to change settings (the frame's delta time, say).  brmi_set_scene keeps
 * the binding.  It refuses with BRMI_ERR_INVALID, before anything is launched: a wrong structSize (buffers or settings), a null scratch or ldr, a scratch or
 * blendedHdr not 16 B aligned, an ldr not 4 B aligned, short buffers, tonemapType > 4, bloom or autoExposure > 1, non-zero reserved words, a non-finite setting
 * or a range <= 0, bloom with a side below 32, and a pass with a row band, dynamicBand or stripes (the histogram is frame-wide, the taps cross rows). */
typedef struct brmi_display_settings {
    uint32_t structSize;        /* sizeof(brmi_display_settings) */
    uint32_t tonemapType;
    uint32_t bloom;
    uint32_t autoExposure;
    float    minLogLuminance;
    float    logLuminanceRange;
    float    timeCoefficient;
    float    fixedAdaptedLuminance;
    uint32_t reserved[4];       /* zero */
} brmi_display_settings;        /* 48 B */
typedef struct brmi_display_plane { uint64_t offset, bytes; uint32_t width, height; } brmi_display_plane;      /* byte offset into the scratch, whole tiles */
typedef struct brmi_display_layout {
    brmi_display_plane bloom[5];        /* levels 1 .. 5 (RGBA16F, tiled); bytes 0 where the frame has fewer levels or bloom is refused */
    uint32_t bloomLevels;               /* 0 where bloom is refused (a side below 32) */
    uint32_t reserved;
    uint64_t histogramOffset;           /* 256 words */
    uint64_t adaptedLuminanceOffset;    /* one float */
    uint64_t controlBlockOffset;        /* 96 words, 128 B aligned */
    uint64_t scratchBytes;              /* what brmi_display_buffers::scratch must hold */
    uint64_t ldrBytes;                  /* W * H * 4 */
    uint64_t blendedHdrBytes;           /* 8 B per pixel, whole tiles */
} brmi_display_layout;                  /* 176 B */
typedef struct brmi_display_buffers {
    uint32_t structSize;        /* sizeof(brmi_display_buffers) */
    uint32_t reserved;
    brmi_display_settings settings;
    void*    scratch;    uint64_t scratchBytes;
    void*    ldr;        uint64_t ldrBytes;
    void*    blendedHdr; uint64_t blendedHdrBytes;      /* NULL: not written.  Written only with bloom on. */
} brmi_display_buffers;         /* 104 B */
void brmi_display_default_settings(brmi_display_settings* settings);
int  brmi_display_get_layout(uint32_t width, uint32_t height, brmi_display_layout* layout);      /* BRMI_ERR_INVALID: a null layout or an empty frame */
int  brmi_set_display(brmi_pass* pass, const brmi_display_buffers* buffers_or_NULL);
/* The stages.  BRMI_ERR_STATE before brmi_setup / brmi_update, or when nothing is bound.  exposure: histogram + average + control block (autoExposure 0: the
 * control block alone); bloom: the down- and upsamples into levels 1 .. 5 (bloom 0: nothing); resolve: blend, tone curve, gamma, the RGBA8 store. */
int  brmi_display_exposure(brmi_pass* pass, brmi_stream stream);
int  brmi_display_bloom(brmi_pass* pass, brmi_stream stream);
int  brmi_display_resolve(brmi_pass* pass, brmi_stream stream);
/* One of the reference's BloomSamplePass{mipIndex, isUpsample} on its own, for tests that hold the pyramid level by level: down (mipIndex 0 .. 4) writes level
 * mipIndex + 1 from level mipIndex, level 0 being the pass's HDR target; up (mipIndex 1 .. 4) adds the tent of level mipIndex + 1 to level mipIndex. */
int  brmi_debug_display_histogram(brmi_pass* pass, brmi_stream stream);      /* LuminanceHistogramPass alone: adds the frame's counts to the histogram */
int  brmi_debug_display_bloom_pass(brmi_pass* pass, uint32_t mipIndex, uint32_t isUpsample, brmi_stream stream);

/* ---- Temporal anti-aliasing: the stage between the lit frame and the display chain, where the reference runs its upscaler ------------------------
 * The caller jitters the main camera's `projection` (brmi_passes.hpp: jitter_offset / jitter_camera; `unjitteredProjection` stays, so the motion plane does not see
 * the jitter); the stage resolves the one-sample frame against last frame's resolved image at native resolution: a 3 x 3 neighbourhood box in w = c / (1 + max c),
 * the motion vector of the closest of the nine pixels, a bilinear history sample, the clamp into the box, r = h + blend * (w(current) - h), the inverse of w.  Where
 * there is no history (none yet, the reprojected position outside the frame, a sample that is not finite) the current colour passes unchanged.  Alpha is carried.
 * Off by default: a pass that never calls brmi_set_temporal, or calls it with NULL, launches exactly what it launched before and writes the same bytes.  With it
 * bound, brmi_execute / brmi_execute_split run brmi_temporal_resolve behind the skybox stage and ahead of the display chain, on the shading stream, and the display
 * stages read the resolved image where they read the HDR target, which this stage never writes.
 *
 * `history[0]`, `history[1]`: two caller-owned images in the surfaces' tiled layout (brmi_temporal_get_layout: 8 B per pixel, whole tiles), 16 B aligned and not
 * overlapping.  The pass reads the one it wrote last and writes the other.  After brmi_set_temporal, brmi_set_scene or brmi_temporal_reset the history is invalid:
 * the next resolve writes the current frame.  Calling brmi_set_temporal again therefore also restarts the accumulation.
 * A binding belongs to ONE pass.  One camera sequence rendered through several passes in flight (brmi_set_history_source) is not supported with a temporal binding:
 * each pass would hold every second frame's history.  brmi_set_temporal refuses a pass that has a history source or is one, and brmi_set_history_source refuses a
 * pass with a temporal binding.
 * Refusals (BRMI_ERR_INVALID, before anything is launched): a wrong structSize (buffers or settings), a null, misaligned or short image, the two images overlapping,
 * blend outside (0, 1] or not finite, phases 0, non-zero reserved words, a pass with a row band, dynamicBand or stripes (the taps cross rows), a history source. */
typedef struct brmi_temporal_settings {
    uint32_t structSize;        /* sizeof(brmi_temporal_settings) */
    float    blend;             /* weight of the current frame, (0, 1]; default 0.1 */
    uint32_t phases;            /* length of the jitter sequence the caller walks (jitter_offset); default 16.  The kernel does not read it. */
    uint32_t reserved[5];       /* zero */
} brmi_temporal_settings;       /* 32 B */
typedef struct brmi_temporal_layout {
    uint64_t historyBytes;      /* one history image: whole tiles, 8 B per pixel */
    uint32_t tilesX, tilesY;
} brmi_temporal_layout;         /* 16 B */
typedef struct brmi_temporal_buffers {
    uint32_t structSize;        /* sizeof(brmi_temporal_buffers) */
    uint32_t reserved;
    brmi_temporal_settings settings;
    void*    history[2];
    uint64_t historyBytes;      /* what EACH image holds */
} brmi_temporal_buffers;        /* 64 B */
void brmi_temporal_default_settings(brmi_temporal_settings* settings);
int  brmi_temporal_get_layout(uint32_t width, uint32_t height, brmi_temporal_layout* layout);      /* BRMI_ERR_INVALID: a null layout or an empty frame */
int  brmi_set_temporal(brmi_pass* pass, const brmi_temporal_buffers* buffers_or_NULL);
int  brmi_temporal_resolve(brmi_pass* pass, brmi_stream stream);      /* the stage alone.  BRMI_ERR_STATE before brmi_setup / brmi_update, or when nothing is bound */
int  brmi_temporal_reset(brmi_pass* pass);                            /* the next resolve has no history */
/* Which of the two images holds the last resolved frame (0 or 1), and whether the next resolve has a history. */
int  brmi_temporal_state(const brmi_pass* pass, uint32_t* resolvedIndex, uint32_t* historyValid);
/* The kernel on caller-given device surfaces in the tiled layout (whole tiles each): hdr and out 8 B, depth and motion 4 B per pixel; history NULL = absent.
 * Needs no pass; a refusal is read with brmi_last_error(NULL). */
int  brmi_debug_temporal_resolve(uint32_t width, uint32_t height, const void* hdr, const void* depth, const void* motion, const void* history_or_NULL, void* out,
                                 const brmi_temporal_settings* settings, brmi_stream stream);

/* Debug views.  brmi_set_debug_view binds the targets (NULL unbinds and gives exactly the frames of a pass that never called it); with a target bound and
 * perFrame.outputType != 0, brmi_execute / brmi_execute_split run brmi_debug_view behind the shading stage (on the shading stream); an outputType the stage
 * would refuse makes them fail BEFORE anything is launched.  The lit HDR frame and
 * every plane are written as always (deferred.hlsl:62-63 does the same): nothing of the frame depends on the mode.  Row bands are supported (only the band's
 * rows are written); the INTERLEAVED partition (brmi_config::stripeCount > 1) is refused, because the pixel rows of its compact surfaces are not the
 * frame's rows and a debug image of them would not be the picture.  Refusals: BRMI_ERR_INVALID for a wrong structSize, a null / misaligned / short
 * payload, a short image, stripes. */
uint64_t brmi_debug_view_bytes(uint32_t width, uint32_t height);
int brmi_set_debug_view(brmi_pass* pass, const brmi_debug_view_buffers* view);
/* The stage: the payload kernel for the outputType of the last brmi_update, then the resolve where an image is bound.  Reads the surfaces of the frame
 * the pass last rendered; returns without a launch for outputType == 0.  BRMI_ERR_STATE before brmi_setup / brmi_update or without a bound target,
 * BRMI_ERR_INVALID for an outputType outside brmi_output_type (or a light-cluster mode without enableClusteredLighting). */
int brmi_debug_view(brmi_pass* pass, brmi_stream stream);

/* Rows [bandY0, bandY1) of the frame this GPU renders FROM THE NEXT FRAME ON (multiples of 8; passes created with brmi_config::dynamicBand): call it between frames,
 * before the frame's brmi_update.  The screen-tile split of SURVEY.md 8(e) with regions whose boundaries follow the cost of the frames before, so that every GPU takes
 * the same time: a cluster is set up by the one GPU whose band holds it (two at a boundary), and the band test of the instance / node / cluster culling drops the rest
 * of the hierarchy.  Launches already enqueued keep the band they were issued with.  The depth chain's texels of rows that leave the band are reset to "empty" by the
 * next chain build, so a stale depth never occludes anything in phase 2. */
int brmi_set_band(brmi_pass* pass, uint32_t bandY0, uint32_t bandY1);

/* ---- stage-level entry points: one per compute pass the reference's graph schedules ---------
 * (order of BR/src/Render/GraphExtensions/CLodExtension.cpp:1580-2088 and
 *  BR/include/Render/RenderGraphBuildHelper.h:220-414) */
int brmi_clear_visibility(brmi_pass* pass, brmi_stream stream);   /* ClearVisibilityBufferPass */
int brmi_cull(brmi_pass* pass, uint32_t phase, brmi_stream stream);       /* HierarchicalCullingPass1/2 (K1-K3) */
int brmi_raster(brmi_pass* pass, uint32_t phase, brmi_stream stream);     /* SoftwareRasterizeClustersPass1/2 (K5) */
int brmi_depth_copy(brmi_pass* pass, brmi_stream stream);         /* LinearDepthCopyPass (K6) */
/* CLodStreamingFeedbackSortPass: compacts and orders what the frame's culling recorded into loadRequests / touchedGroups / counts.  brmi_execute runs it after the
 * frame's last culling phase, brmi_execute_split on the geometry stream; the frame's first culling launch resets the per-frame state (CLodStreamingBeginFramePass).
 * BRMI_ERR_STATE without brmi_set_streaming. */
int brmi_streaming_feedback(brmi_pass* pass, brmi_stream stream);
int brmi_build_hzb(brmi_pass* pass, brmi_stream stream);          /* LinearDepthDownsamplePass (SPD max-reduce; BR/shaders/downsample.hlsl) */
/* Drops the previous frame's depth chain (camera cut, resize): the next phase 1 runs without occlusion tests. */
int brmi_invalidate_hzb(brmi_pass* pass);
/* Frames in flight (the reference's `numFramesInFlight`, CLodStreamingSystem.cpp:956): two passes with their own resources render
 * alternate frames on two streams; phase 1 of a pass then tests against the depth chain the OTHER pass built for the frame before
 * (`source`), not against its own, which is two frames old.  Both passes must have the same size and band; for two frames in
 * flight each is the other's source.  brmi_execute orders the streams itself: a frame starts when the source's chain of the frame before is complete
 * (one event wait), everything after the source's chain build -- its G-buffer and shading -- overlaps this pass's culling and
 * rasterisation.  The images are those of one pass rendering the same frames in order.  NULL unlinks. */
int brmi_set_history_source(brmi_pass* pass, brmi_pass* source);
int brmi_gbuffer(brmi_pass* pass, brmi_stream stream);            /* MaterialHistogram..EvaluateMaterialGroups (K7,K8) */
int brmi_light_clustering(brmi_pass* pass, brmi_stream stream);   /* ClusterGenerationPass + LightCullingPass (K9,K10) */
int brmi_shade(brmi_pass* pass, brmi_stream stream);              /* DeferredShadingPass (K11) */
/* Shading in row slabs (multi-GPU composition overlapped with the frame's own shading): with slabs > 1 the deferred-shading launches of
 * brmi_shade / brmi_execute / brmi_execute_split cover the band in that many slabs of rows (multiples of 8 surface rows, top to bottom), and
 * `fn(user, row0, row1, stream)` is called on the host right after a slab's launches have been enqueued on `stream` -- the place to hand the rows
 * to brmi_compose_submit_rows (include/brmi_compose.h), whose stores then travel while the next slab is shaded.  Same pixels, same bytes as
 * one launch over the band.  slabs <= 1 or fn == NULL: one launch, no call. */
typedef void (*brmi_slab_fn)(void* user, uint32_t row0, uint32_t row1, brmi_stream stream);
int brmi_set_shade_slabs(brmi_pass* pass, uint32_t slabs, brmi_slab_fn fn, void* user);

/* ---- introspection ------------------------------------------------------------------------- */
int brmi_read_counters(brmi_pass* pass, brmi_counters* out, brmi_stream stream);   /* synchronises */
/* mean milliseconds per stage AND FRAME over the frames executed since the previous call (at most the last 32; the depth-chain stage, which
 * brmi_execute runs twice per frame, reports the sum of its two builds;
 * HIP events on the execute stream, collectPassStatistics); synchronises and resets the window */
int brmi_stage_times(brmi_pass* pass, float* msOut /* [BRMI_STAGE_COUNT] */);
/* Restricts the event pairs to the stages whose bit (1 << brmi_stage) is set; every event pair is a barrier on the stream,
 * so a benchmark times all stages once and then only the one it reports on.  Default: all stages. */
int brmi_set_timed_stages(brmi_pass* pass, uint32_t stageMask);
/* algorithmic bytes of the last frame per SURVEY.md 8(d): 140*P + sum(144+12V+3T) + 64*M + 16*Mvis + 64*N.  A read-back call: waits for
 * the device (whatever stream the frame ran on) before it reads the frame's counters. */
int brmi_algorithmic_bytes(brmi_pass* pass, uint64_t* perStage /* [BRMI_STAGE_COUNT] */, uint64_t* total);
/* The same count for the kernel variants the frame actually LAUNCHED: where a scene lets a stage move less than SURVEY.md 8(d)'s figure, this says how much it is
 * obliged to move -- today one case: no material of the scene has a coat or a fuzz layer, so the shading pass does not read those two G-buffer planes (44 instead of
 * 60 B per pixel).  brmi_algorithmic_bytes stays 8(d)'s definition; a roofline fraction against THIS count is the honest one for the launched kernel. */
int brmi_algorithmic_bytes_launched(brmi_pass* pass, uint64_t* perStage /* [BRMI_STAGE_COUNT] */, uint64_t* total);

/* ---- diagnostics ---------------------------------------------------------------------------- */
/* Evaluates the library's fp32 primitives on device data so a test can check the arithmetic contract
 * (correctly rounded a/b and sqrt(a), round-to-nearest-even float->half) against IEEE on the host. */
int brmi_debug_arith(const float* a, const float* b, float* outDiv, float* outSqrt, uint32_t* outHalfBits, uint32_t n, brmi_stream stream);

/* Triangles of the last frame whose bin records were many enough (more than BRMI_TUNING wide_entries = 128 bins; 16 for the triangles the lean rasteriser queues,
 * lean_wide_entries) to be handed to the cooperative emission pass (k_raster_wide): phase 1's draw pass, its late pass, phase 2.  Counted whether or not the pass
 * was launched (the host launches it while the frames before had such triangles).  Waits for the device. */
int brmi_debug_wide_triangles(brmi_pass* pass, uint32_t out[3]);
/* Round 6, the lean rasteriser: out[0] = 1 when the last frame's phase-1 main launch was the lean form of k_raster (frames of very many clusters;
 * BRMI_TUNING lean_min_clusters), out[1] = how many of its clusters it left to the general launch behind it (skinned vertices, a full triangle queue), out[2] / out[3] =
 * triangles it queued for k_raster_emit (large enough for the bins) and the runs they were queued in (one per wave and pass; requested, so beyond a full queue's
 * capacity).  Waits for the device. */
int brmi_debug_lean_clusters(brmi_pass* pass, uint32_t out[4]);
/* The register shape of the opaque direct rasteriser the last frame's phase 1 launched: *slim = 1 when one of its k_raster launches (the main one, the
 * one behind a lean launch, the late pass) was the slim shape (at most 104 VGPRs: a frame issued
 * on two streams by brmi_execute_split, or BRMI_TUNING raster_slim=1), 0 for the general one (one stream, the stage entry point brmi_raster, raster_slim=0, or a scene
 * with alpha-tested materials, which has no slim shape).  Host state only: does not wait for the device. */
int brmi_debug_raster_shape(brmi_pass* pass, uint32_t* slim);
/* One of the 64 stripes of that queue as the last frame left it: counts = {entries, runs} (clamped to the stripe's capacity); runs = {first entry, count} pairs,
 * entries = 96 B records (brmi_raster.hip, WideTri: a 64 B bin record of the triangle's first row, then yHi, band0, band1, strip0, strip1).  Either buffer may be null. */
int brmi_debug_read_lean_queue(brmi_pass* pass, uint32_t stripe, uint32_t* runs, uint32_t maxRuns, void* entries, uint32_t maxEntries, uint32_t counts[2]);

/* The last frame's draw-list decisions, for tests (waits for the device): indices into the visible-cluster buffer of the phase-1 clusters the culling held back
 * (`held`, up to heldCapacity entries; *heldCount = how many there were) and of those the late pass drew (`late`).  held minus late was never rasterised. */
int brmi_debug_read_held(brmi_pass* pass, uint32_t* held, uint32_t heldCapacity, uint32_t* heldCount, uint32_t* late, uint32_t lateCapacity, uint32_t* lateCount);
/* The other side of those decisions (waits for the device): the draw list -- indices of the phase-1 clusters the rasteriser took first (`draw`; *drawCount = the
 * list's counter as the frame left it, unclamped) -- and, in the order of brmi_debug_read_held's `held`, the index of each held record's box in the library's
 * per-meshlet box table (`heldBoxes`; *boxCount = the table's size when asked for).  draw and held partition the placed phase-1 clusters.  Buffers may be null. */
int brmi_debug_read_draw_list(brmi_pass* pass, uint32_t* draw, uint32_t drawCapacity, uint32_t* drawCount, uint32_t* heldBoxes, uint32_t heldCapacity, uint32_t* heldCount, uint32_t* boxCount);

/* Diagnostics: the first `bytes` of the raster bin-record region of the workspace; with bit 62 of `bytes` set, those bytes are zeroed instead (a following
 * frame's records can then be told from older ones).  Waits for the device. */
int brmi_debug_read_bin_records(brmi_pass* pass, void* dst, uint64_t bytes);

/* The shading pass's in-range forms of 1 / a, sqrt(a) and 1 / sqrt(a) (brmi_device.h: the IEEE expansions without their scaling prologue and
 * fix-up epilogue for 2^-63 <= a < 2^63, the general form elsewhere): a test compares them bit for bit with the host's IEEE results. */
int brmi_debug_arith_in_range(const float* a, float* outRcp, float* outSqrt, float* outRsqrt, uint32_t n, brmi_stream stream);


/* The G-buffer pass's SampleGrad on device data, one lane per sample, through the very device function the kernel calls (the texel tables staged in LDS as
 * there): a test compares it bit for bit with the host's statement of the sampler.  Of `scene` only textures / samplers / their counts / srgbToLinear are
 * read.  maxAnisotropy: the table of brmi_set_sampler_anisotropy (samplerCount words), or NULL for the isotropic SampleGrad.  uniformBinding = 1 fetches the
 * descriptors through the constant address space as the kernel's waterfall path does (the power-of-two fast path is reachable), 0 binds per lane (the
 * general path).  uv / ddx / ddy: n float2 each; outRGBA: n float4.  Every pointer is a device pointer. */
int brmi_debug_sample_grad(const brmi_scene_buffers* scene, const uint32_t* maxAnisotropy /* device, or NULL */, uint32_t textureIndex,
                           uint32_t samplerIndex, uint32_t uniformBinding, const float* uv, const float* ddx, const float* ddy, float* outRGBA,
                           uint32_t n, brmi_stream stream);

/* The shading pass's environment term on device data, one lane per sample, through the device functions k_shade_ibl calls.  Every pointer
 * but `env` (a host struct of device pointers, as brmi_set_environment takes it) is a device pointer.
 * brmi_debug_ibl_lookup: the cube lookup alone.  directions: n float3, lods: n floats, outRGBA: n float4 = SampleLevel(g_linearClamp, direction, lod) of cubemap
 *   `cubemapIndex` of env->cubemaps.
 * brmi_debug_ibl: the whole term of n made-up pixels.  The G-buffer words are those a RawPixel holds (normals: n float4 with the OpenPBR record's index in w;
 *   albedo / metallicRoughness: n packed UNORM words; coat / emissive / fuzz: n words of four halves), viewWS: n float3, the unit vector towards the eye.  The
 *   OpenPBR records, lookup tables and per-material shading tables are those of `pass` (after brmi_setup and a brmi_update: the call builds the frame constants
 *   if the pass has not yet), the environment is entry `environmentIndex` of `env`, which need not be bound to the pass.  outDiffuse / outSpecular: n float3
 *   each, fp32: Fd and Fr + coatFr + fuzzFr, the reference's diffuseIBL / specularIBL split. */
int brmi_debug_ibl_lookup(const brmi_environment_buffers* env, uint32_t cubemapIndex, const float* directions, const float* lods, float* outRGBA, uint32_t n,
                          brmi_stream stream);
int brmi_debug_ibl(brmi_pass* pass, const brmi_environment_buffers* env, uint32_t environmentIndex, const float* normals, const uint32_t* albedo,
                   const uint32_t* metallicRoughness, const uint64_t* coat, const uint64_t* emissive, const uint64_t* fuzz, const float* viewWS,
                   float* outDiffuse, float* outSpecular, uint32_t n, brmi_stream stream);
/* The cube lookup of the environment build and the skybox stage, which honours the format of the face descriptor it lands on (RGBA16_FLOAT: halves decoded exactly;
 * anything else: the RGBA8 path of brmi_debug_ibl_lookup).  Arguments as brmi_debug_ibl_lookup's, the table given directly; those stages call it with lod 0. */
int brmi_debug_env_lookup(const brmi_texture_desc* cubemaps, uint32_t cubemapCount, uint32_t cubemapIndex, const float* directions, const float* lods,
                          float* outRGBA, uint32_t n, brmi_stream stream);

/* ---- shadow maps of spot and point lights --------------------------------------------------------------------------------------------------
 * The `GetRootEnableShadows()` block of the light loop (BR/shaders/Include/lighting.hlsli:536-560) for its point and spot branches: calculatePointShadow and
 * calculateSpotShadow of BR/shaders/Include/shadows.hlsli, restated as written.  The directional branch (virtual shadow maps) is not built: a directional light
 * is never shadowed, whatever its fields say.
 *   maps                device array of brmi_texture_desc, BRMI_TEXTURE_FORMAT_R32_FLOAT, one level each.  A spot light's shadowMapIndex names one descriptor; a
 *                       point light's names the first of six consecutive square faces in the order +X -X +Y -Y +Z -Z.
 *   spotCameraIndices   Builtin::Light::SpotLightMatrixBuffer: entry light.shadowViewInfoIndex is the light view's index in brmi_scene_buffers::cameras.
 *   pointCameraIndices  Builtin::Light::PointLightCubemapBuffer: entries light.shadowViewInfoIndex * 6 + face, six per light (pointCount counts lights).
 * The cameras named here are read from the CALLER's camera buffer (not from the frame's snapshot of the main camera): they stay as they are while a frame
 * that reads them is in flight, like the lights and the maps.
 * A light whose shadowViewInfoIndex or shadowMapIndex is -1 is unshadowed.  The lookup is a plain bilinear fetch of level 0: fp32 weights, a tap outside a
 * spot map reads the border value 1.0; a cube takes the face, the texel addresses and the edge rule of the environment cube lookup.
 * brmi_set_shadows reads the lights, the descriptors and the index arrays back once and refuses with BRMI_ERR_INVALID: a wrong structSize, a null table with a
 * non-zero count, a shadowed spot / point light whose shadowMapIndex (+ 5 for a point light) is outside `maps` or whose shadowViewInfoIndex is outside its
 * index array, a spot or point view index >= cameraCount, and a descriptor whose format is not R32_FLOAT (or that has no texels, no size or more than one level).
 * NULL unbinds and gives exactly the frames -- kernels, bytes -- of a pass that never called it.  brmi_set_scene forgets the binding (it is validated against
 * the scene's lights and cameras). */
typedef struct brmi_shadow_buffers {
    uint32_t structSize;                        /* sizeof(brmi_shadow_buffers) */
    uint32_t reserved;
    const brmi_texture_desc* maps;              uint32_t mapCount;    uint32_t reserved0;
    const uint32_t*          spotCameraIndices; uint32_t spotCount;   uint32_t reserved1;
    const uint32_t*          pointCameraIndices; uint32_t pointCount; uint32_t reserved2;
} brmi_shadow_buffers;                          /* 56 B */
int brmi_set_shadows(brmi_pass* pass, const brmi_shadow_buffers* buffers_or_NULL);
/* A light view's depth as the shadow map the shader samples.  `lightPass` has rendered the view (clear, cull, raster, depth copy).  brmi_depth_copy MUST have
 * run: the kernel reads the depth surface alone and takes the "empty" word that stage writes for an empty visibility key as background.  It reads the pass's tiled
 * linear depth (BRMI_RES_LINEAR_DEPTH) and writes dst->texels (device, R32_FLOAT, row-major, dst->width x dst->height = the pass's frame; `dst` is a HOST struct):
 * 1.0f for a pixel without geometry, else d = zFar * (z - zNear) / (z * (zFar - zNear)) in fp32 in that order -- what the reference's light projection
 * (XMMatrixPerspectiveFovRH(.., nearPlane, farPlane)) leaves in its depth target, the inverse of the shader's unprojectDepth. */
int brmi_shadow_capture(brmi_pass* lightPass, float zNear, float zFar, const brmi_texture_desc* dst, brmi_stream stream);
/* The shadow function of light `lightIndex` (an index into brmi_scene_buffers::lights) alone, for n made-up receivers: positionsWS / normalsWS n float3 each,
 * outShadow n floats (1 = shadowed, 0 = lit or unshadowed light), all device pointers.  The device function is the one the shading kernels call.  Needs a
 * binding (BRMI_ERR_STATE without one). */
int brmi_debug_shadow(brmi_pass* pass, uint32_t lightIndex, const float* positionsWS, const float* normalsWS, float* outShadow, uint32_t n, brmi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* BRMI_H */
