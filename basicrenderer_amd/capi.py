"""ctypes mirrors of include/brmi.h, include/brmi_scene.h and loaders for the in-tree libraries.

Harness-side plumbing only: the product is libbrmi.so (HIP kernels behind the C ABI).  This module
never imports anything from oracle/.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

u32, u64, f32, vp = C.c_uint32, C.c_uint64, C.c_float, C.c_void_p


class SceneParams(C.Structure):
    _fields_ = [("preset", u32), ("seed", u32), ("width", u32), ("height", u32), ("numPointLights", u32),
                ("withDirectionalLight", u32), ("lodLevels", u32), ("sizeScale", f32), ("skinnedFraction1024", u32),
                ("materialFeatures", u32), ("cameraStep", u32), ("lodBuilder", u32), ("spotLightEvery", u32), ("detail", f32), ("uniqueTriangleBudget", u32), ("reliefSlope", f32)]


class MeshInput(C.Structure):
    _fields_ = [("positions", vp), ("normals", vp), ("uvs", vp), ("colors", vp), ("vertexCount", C.c_size_t), ("indices", vp), ("indexCount", C.c_size_t),
                ("material", u32), ("reserved", u32 * 3)]


class InstanceInput(C.Structure):
    _fields_ = [("mesh", u32), ("reverseWinding", u32), ("model", (f32 * 4) * 4)]


class ViewInput(C.Structure):
    _fields_ = [("eye", f32 * 3), ("yaw", f32), ("pitch", f32), ("fovYDegrees", f32), ("zNear", f32), ("zFar", f32)]


class DagGroup(C.Structure):
    _fields_ = [("depth", C.c_int32), ("center", f32 * 3), ("radius", f32), ("error", f32), ("firstCluster", u32), ("clusterCount", u32)]


class DagCluster(C.Structure):
    _fields_ = [("group", C.c_int32), ("refined", C.c_int32), ("center", f32 * 3), ("radius", f32), ("error", f32),
                ("vertexCount", u32), ("triangleCount", u32), ("firstVertex", u32), ("firstTriangleByte", u32)]


class Dag(C.Structure):
    """brmi_dag (include/brmi_scene.h): a cluster-LOD DAG as flat arrays."""
    _fields_ = [("groups", C.POINTER(DagGroup)), ("groupCount", u32), ("clusters", C.POINTER(DagCluster)), ("clusterCount", u32),
                ("vertexRefs", C.POINTER(u32)), ("vertexRefCount", u32), ("triangles", C.POINTER(C.c_uint8)), ("triangleBytes", u32), ("owner", vp)]


LOD_BUILDERS = {"quadtree": 0, "external": 1, "own": 2}


class SceneStats(C.Structure):
    _fields_ = [("uniqueTriangles", u64), ("instancedTriangles", u64)] + \
               [(n, u32) for n in ("meshes instances meshletsTotal meshletsLod0 pages nodes groups segments "
                                   "lights materials maxBvhDepth lodLevelsMax").split()] + \
               [("sceneMin", f32 * 3), ("sceneMax", f32 * 3)]


# order == enum brmi_scene_array
SCENE_ARRAYS = ["perObject", "normalMatrices", "perMesh", "perMeshInstance", "clodOffsets", "meshMetadata", "lodNodes",
                "lodGroups", "lodSegments", "groupPageMap", "materials", "openpbrMaterials", "lights",
                "activeLightIndices", "cameras", "cullingCameras", "viewRasterInfo", "perFrame", "activeDraws",
                "skinningMatrices", "lutOdE", "lutOdAvg", "lutImE", "lutImAvg", "lutFuzzLTC",
                "textureDescs", "texels", "samplerDescs", "srgbToLinear"]


class SceneBuffers(C.Structure):
    """brmi_scene_buffers (include/brmi.h).  Pointers are host or device addresses."""
    _fields_ = [
        ("slabs", vp), ("slabCount", u32),
        ("perObject", vp), ("perObjectCount", u32),
        ("normalMatrices", vp),
        ("perMesh", vp), ("perMeshCount", u32),
        ("perMeshInstance", vp), ("perMeshInstanceCount", u32),
        ("clodOffsets", vp),
        ("meshMetadata", vp), ("meshMetadataCount", u32),
        ("lodNodes", vp), ("lodNodeCount", u32),
        ("lodGroups", vp), ("lodGroupCount", u32),
        ("lodSegments", vp), ("lodSegmentCount", u32),
        ("groupPageMap", vp), ("groupPageMapCount", u32),
        ("materials", vp), ("materialCount", u32),
        ("openpbrMaterials", vp), ("openpbrMaterialCount", u32),
        ("lights", vp), ("lightCount", u32),
        ("activeLightIndices", vp),
        ("cameras", vp), ("cameraCount", u32),
        ("cullingCameras", vp),
        ("viewRasterInfo", vp),
        ("perFrame", vp),
        ("activeDraws", vp), ("activeDrawCount", u32),
        ("skinningMatrices", vp), ("skinningMatrixCount", u32),
        ("lutOpaqueDielectricEnergyComplement", vp),
        ("lutOpaqueDielectricAvgEnergyComplement", vp),
        ("lutIdealMetalEnergyComplement", vp),
        ("lutIdealMetalAvgEnergyComplement", vp),
        ("lutFuzzLTC", vp),
        ("textures", vp), ("textureCount", u32),
        ("samplers", vp), ("samplerCount", u32),
        ("srgbToLinear", vp),
    ]


class Config(C.Structure):
    _fields_ = [("structSize", u32), ("width", u32), ("height", u32), ("maxVisibleClusters", u32),
                ("maxTraversalRecords", u32), ("enableOcclusionCulling", u32), ("enableClusteredLighting", u32),
                ("enablePunctualLights", u32), ("lightClusterSize", u32 * 3), ("phase2ExpansionFactor", u32),
                ("collectPassStatistics", u32), ("maxBvhLevels", u32), ("bandY0", u32), ("bandY1", u32),
                ("keepUniformLayerPlanes", u32), ("stripeRows", u32), ("stripeCount", u32), ("stripeIndex", u32), ("fullHeight", u32), ("dynamicBand", u32), ("reserved", u32 * 2)]


class ResourceDesc(C.Structure):
    _fields_ = [("id", u32), ("name", C.c_char_p), ("bytes", u64), ("usage", u32), ("width", u32), ("height", u32),
                ("bytesPerPixel", u32), ("tileW", u32), ("tileH", u32)]


class ResourceBinding(C.Structure):
    _fields_ = [("id", u32), ("ptr", vp), ("bytes", u64)]


class FrameUpdate(C.Structure):
    _fields_ = [("mainCameraHost", vp), ("perFrameHost", vp), ("frameIndex", u32)]


class StreamingBuffers(C.Structure):
    """brmi_streaming_buffers (include/brmi.h): caller-owned device memory of the residency-aware cut and its feedback."""
    _fields_ = [("structSize", u32), ("activeGroupScanCount", u32), ("nonResidentBits", vp), ("loadRequests", vp), ("requestCapacity", u32),
                ("touchedGroups", vp), ("touchedCapacity", u32), ("counts", vp), ("scratch", vp), ("scratchBytes", u64)]


class DebugViewBuffers(C.Structure):
    """brmi_debug_view_buffers (include/brmi.h): caller-owned targets of the debug view."""
    _fields_ = [("structSize", u32), ("reserved", u32), ("payload", vp), ("payloadBytes", u64), ("image", vp), ("imageBytes", u64)]


class GtaoSettings(C.Structure):
    """brmi_gtao_settings (include/brmi.h), 32 B."""
    _fields_ = [("structSize", u32), ("qualityLevel", u32), ("denoisePasses", u32), ("radius", f32), ("maxDepthLod", u32), ("reserved", u32 * 3)]


class GtaoPlane(C.Structure):
    _fields_ = [("offset", u64), ("width", u32), ("height", u32)]


class GtaoLayout(C.Structure):
    """brmi_gtao_layout (include/brmi.h): where the planes of XeGTAO lie in the caller's scratch, 144 B."""
    _fields_ = [("depth", GtaoPlane * 5), ("edges", GtaoPlane), ("term", GtaoPlane * 2), ("scratchBytes", u64), ("outputBytes", u64)]


class GtaoBuffers(C.Structure):
    """brmi_gtao_buffers (include/brmi.h): the settings and the caller-owned device memory of XeGTAO, 72 B."""
    _fields_ = [("structSize", u32), ("reserved", u32), ("settings", GtaoSettings), ("scratch", vp), ("scratchBytes", u64), ("aoTerm", vp), ("aoTermBytes", u64)]


class DisplaySettings(C.Structure):
    """brmi_display_settings (include/brmi.h), 48 B."""
    _fields_ = [("structSize", u32), ("tonemapType", u32), ("bloom", u32), ("autoExposure", u32), ("minLogLuminance", f32), ("logLuminanceRange", f32),
                ("timeCoefficient", f32), ("fixedAdaptedLuminance", f32), ("reserved", u32 * 4)]


class DisplayPlane(C.Structure):
    _fields_ = [("offset", u64), ("bytes", u64), ("width", u32), ("height", u32)]


class DisplayLayout(C.Structure):
    """brmi_display_layout (include/brmi.h): where the display chain's state and bloom levels lie in the caller's scratch, 176 B."""
    _fields_ = [("bloom", DisplayPlane * 5), ("bloomLevels", u32), ("reserved", u32), ("histogramOffset", u64), ("adaptedLuminanceOffset", u64),
                ("controlBlockOffset", u64), ("scratchBytes", u64), ("ldrBytes", u64), ("blendedHdrBytes", u64)]


class DisplayBuffers(C.Structure):
    """brmi_display_buffers (include/brmi.h): the settings and the caller-owned device memory of the display chain, 104 B."""
    _fields_ = [("structSize", u32), ("reserved", u32), ("settings", DisplaySettings), ("scratch", vp), ("scratchBytes", u64), ("ldr", vp), ("ldrBytes", u64),
                ("blendedHdr", vp), ("blendedHdrBytes", u64)]


class TemporalSettings(C.Structure):
    """brmi_temporal_settings (include/brmi.h), 32 B."""
    _fields_ = [("structSize", u32), ("blend", f32), ("phases", u32), ("reserved", u32 * 5)]


class TemporalLayout(C.Structure):
    """brmi_temporal_layout (include/brmi.h): the bytes of one history image, 16 B."""
    _fields_ = [("historyBytes", u64), ("tilesX", u32), ("tilesY", u32)]


class TemporalBuffers(C.Structure):
    """brmi_temporal_buffers (include/brmi.h): the settings and the two caller-owned history images, 64 B."""
    _fields_ = [("structSize", u32), ("reserved", u32), ("settings", TemporalSettings), ("history", vp * 2), ("historyBytes", u64)]


TONEMAP_TYPES = {"reinhard": 0, "neutral": 1, "aces": 2, "lpm": 3, "none": 4}      # the reference's tonemapType setting; 4 is the switch's default
GTAO_QUALITY = {"low": 0, "medium": 1, "high": 2, "ultra": 3}      # slices x steps: 1 x 2, 2 x 2, 3 x 3, 9 x 3


class EnvironmentInfo(C.Structure):
    """brmi_environment_info (include/brmi_types.h): the reference's EnvironmentInfo, 128 B."""
    _fields_ = [("cubeMapDescriptorIndex", u32), ("prefilteredCubemapDescriptorIndex", u32), ("sphericalHarmonicsScale", f32),
                ("sphericalHarmonics", C.c_int32 * 27), ("pad", u32 * 2)]


class EnvironmentBuffers(C.Structure):
    """brmi_environment_buffers (include/brmi.h): caller-owned device tables of the image-based lighting."""
    _fields_ = [("structSize", u32), ("specularIBL", u32), ("environments", vp), ("environmentCount", u32), ("reserved0", u32), ("cubemaps", vp), ("cubemapCount", u32),
                ("reserved1", u32), ("skybox", u32), ("reserved2", u32 * 3)]


class EnvironmentBuffersV1(C.Structure):
    """brmi_environment_buffers as it was before `skybox` (BRMI_ENVIRONMENT_BUFFERS_SIZE_V1 bytes): still accepted, and means skybox off."""
    _fields_ = [("structSize", u32), ("specularIBL", u32), ("environments", vp), ("environmentCount", u32), ("cubemaps", vp), ("cubemapCount", u32)]


class TextureDesc(C.Structure):
    """brmi_texture_desc (include/brmi_types.h), 96 B."""
    _fields_ = [("texels", vp), ("width", u32), ("height", u32), ("mipCount", u32), ("format", u32), ("mipOffset", u32 * 16), ("reserved", u32 * 2)]


class MaterialInputs(C.Structure):
    """brmi_material_inputs (include/brmi_scene.h)."""
    _fields_ = [("structSize", u32), ("reserved", u32), ("materials", vp), ("materialCount", u32), ("openpbrCount", u32), ("openpbr", vp),
                ("textures", vp), ("textureCount", u32), ("samplerCount", u32), ("samplers", vp), ("uvs1", vp)]


class ShadowBuffers(C.Structure):
    """brmi_shadow_buffers (include/brmi.h): caller-owned device tables of the spot / point shadow maps, 56 B."""
    _fields_ = [("structSize", u32), ("reserved", u32), ("maps", vp), ("mapCount", u32), ("reserved0", u32), ("spotCameraIndices", vp), ("spotCount", u32),
                ("reserved1", u32), ("pointCameraIndices", vp), ("pointCount", u32), ("reserved2", u32)]


TEXTURE_FORMAT_RGBA8_UNORM, TEXTURE_FORMAT_RGBA8_UNORM_SRGB, TEXTURE_FORMAT_RGBA16_FLOAT = 0, 1, 2      # BRMI_TEXTURE_FORMAT_*
TEXTURE_FORMAT_R32_FLOAT = 3
TEXTURE_MAX_MIPS = 16
ENVIRONMENT_BUFFERS_SIZE_V1 = 40


SH_FLOAT_SCALE = 100                      # BRMI_SH_FLOAT_SCALE
PER_FRAME_ACTIVE_ENVIRONMENT_WORD = 11    # brmi_per_frame::activeEnvironmentIndex as a u32 index

# perFrame.outputType values with a payload kernel (brmi_output_type; the reference's OUTPUT_* names without the prefix)
OUTPUT_TYPES = {"COLOR": 0, "NORMAL": 1, "ALBEDO": 2, "METALLIC": 3, "ROUGHNESS": 4, "EMISSIVE": 5, "AO": 6, "DEPTH": 7, "MESHLETS": 10,
                "LIGHT_CLUSTER_ID": 12, "LIGHT_CLUSTER_LIGHT_COUNT": 13, "MOTION_VECTORS": 14, "GEOMETRY_GROUP": 35}
PER_FRAME_OUTPUT_TYPE_WORD = 12      # brmi_per_frame::outputType as a u32 index


class Counters(C.Structure):
    _fields_ = [(n, u32) for n in ("instancesTested instancesVisible nodesVisited bucketRecords meshletsTested "
                                   "visibleClusters visibleClustersPhase2 droppedRecords droppedClusters "
                                   "lightPagesUsed replayNodes replayMeshlets").split()] + [("reserved", u32 * 6)]


class ComposeConfig(C.Structure):
    """brmi_compose_config (include/brmi_compose.h)."""
    _fields_ = [("structSize", u32), ("width", u32), ("bandY0", u32), ("bandY1", u32), ("bytesPerPixel", u32), ("transport", u32), ("depth", u32),
                ("rank", u32), ("nRanks", u32), ("device", C.c_int32), ("path", u32), ("waitTimeoutMs", u32), ("frameHeight", u32), ("reserved", u32 * 3)]


COMPOSE_EXPORTS = ["brmi_compose_unique_id", "brmi_compose_create", "brmi_compose_staging_bytes", "brmi_compose_output_bytes", "brmi_compose_bind",
                   "brmi_compose_submit", "brmi_compose_finish", "brmi_compose_destroy", "brmi_compose_last_error",
                   "brmi_compose_alloc_shared", "brmi_compose_export", "brmi_compose_import", "brmi_compose_last_wait_status", "brmi_compose_submit_rows", "brmi_compose_wait_source", "brmi_compose_set_bounds", "brmi_compose_balance_rows"]
COMPOSE_HANDLE_BYTES = 160
_compose_lib = None


def compose_lib():
    """libbrmi_compose.so: RCCL composition of the row-band partition behind a C ABI.  torch is imported first so that its RCCL / HIP
    runtime (same SONAMEs) are the ones the process uses."""
    global _compose_lib
    if _compose_lib is None:
        import torch  # noqa: F401
        path = os.path.join(LIB_DIR, "libbrmi_compose.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make compose` (or __graft_entry__.build())")
        try:      # torch ships librccl.so without the .1 suffix: map it under its SONAME before the library asks for it
            C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so"), mode=C.RTLD_GLOBAL)
        except OSError:
            pass
        lib = C.CDLL(path)
        lib.brmi_compose_unique_id.argtypes = [vp]
        lib.brmi_compose_create.argtypes = [C.POINTER(ComposeConfig), C.c_char_p, C.POINTER(vp)]
        lib.brmi_compose_staging_bytes.argtypes = [vp]
        lib.brmi_compose_staging_bytes.restype = u64
        lib.brmi_compose_output_bytes.argtypes = [vp]
        lib.brmi_compose_output_bytes.restype = u64
        lib.brmi_compose_bind.argtypes = [vp, vp, u64, vp, u64]
        lib.brmi_compose_submit.argtypes = [vp, vp, vp]
        lib.brmi_compose_finish.argtypes = [vp, vp, C.POINTER(vp)]
        lib.brmi_compose_destroy.argtypes = [vp]
        lib.brmi_compose_alloc_shared.argtypes = [vp]
        lib.brmi_compose_export.argtypes = [vp, C.c_char_p]
        lib.brmi_compose_import.argtypes = [vp, C.c_char_p, u32]
        lib.brmi_compose_last_wait_status.argtypes = [vp]
        lib.brmi_compose_submit_rows.argtypes = [vp, vp, u32, u32, vp]
        lib.brmi_compose_wait_source.argtypes = [vp, vp, vp]; lib.brmi_compose_wait_source.restype = C.c_int
        lib.brmi_compose_destroy.restype = None
        lib.brmi_compose_last_error.argtypes = [vp]
        lib.brmi_compose_last_error.restype = C.c_char_p
        _compose_lib = lib
    return _compose_lib


DECLARE_CB = C.CFUNCTYPE(None, vp, C.POINTER(ResourceDesc))

RES_NAMES = ["VISIBILITY", "LINEAR_DEPTH", "GBUF_NORMALS", "GBUF_ALBEDO", "GBUF_COAT", "GBUF_EMISSIVE", "GBUF_FUZZ",
             "GBUF_METALLIC_ROUGHNESS", "GBUF_MOTION_VECTORS", "HDR_COLOR", "VISIBLE_CLUSTERS", "LIGHT_CLUSTERS",
             "LIGHT_PAGES", "HZB", "WORKSPACE"]
RES = {n: i for i, n in enumerate(RES_NAMES)}
STAGE_NAMES = ["clear", "cull", "raster", "depth_copy", "hzb", "cull2", "raster2", "gbuffer", "light_cluster", "shade"]

_scene_lib = None
_brmi_lib = None


def scene_lib():
    """libbrmi_scene.so: the host-side procedural scene generator."""
    global _scene_lib
    if _scene_lib is None:
        path = os.path.join(LIB_DIR, "libbrmi_scene.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make scene` (or __graft_entry__.build())")
        lib = C.CDLL(path)
        lib.brmi_scene_create.restype = vp
        lib.brmi_scene_create.argtypes = [C.POINTER(SceneParams)]
        lib.brmi_scene_create_with_dag_builder.restype = vp
        lib.brmi_scene_create_with_dag_builder.argtypes = [C.POINTER(SceneParams), vp, vp, vp]
        lib.brmi_scene_create_from_meshes.restype = vp
        lib.brmi_scene_create_from_meshes.argtypes = [C.POINTER(SceneParams), C.POINTER(MeshInput), u32, C.POINTER(InstanceInput), u32, C.POINTER(ViewInput), vp, vp, vp]
        lib.brmi_scene_create_from_meshes_with_materials.restype = vp
        lib.brmi_scene_create_from_meshes_with_materials.argtypes = [C.POINTER(SceneParams), C.POINTER(MeshInput), u32, C.POINTER(InstanceInput), u32, C.POINTER(ViewInput),
                                                                      C.POINTER(MaterialInputs), vp, vp, vp]
        lib.brmi_lod_build.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.POINTER(Dag)]
        lib.brmi_lod_release.argtypes = [vp, C.POINTER(Dag)]
        lib.brmi_lod_release.restype = None
        lib.brmi_scene_create_from_cache.restype = vp
        lib.brmi_scene_create_from_cache.argtypes = [C.POINTER(SceneParams), C.c_char_p]
        lib.brmi_scene_export_cache.argtypes = [vp, C.c_char_p]
        lib.brmi_scene_destroy.argtypes = [vp]
        lib.brmi_scene_array.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u32)]
        lib.brmi_scene_slab_count.argtypes = [vp]
        lib.brmi_scene_slab_count.restype = u32
        lib.brmi_scene_slab.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u64)]
        lib.brmi_scene_get_stats.argtypes = [vp, C.POINTER(SceneStats)]
        lib.brmi_scene_camera_at.argtypes = [C.POINTER(SceneParams), C.c_double, C.c_double, vp, vp]
        _scene_lib = lib
    return _scene_lib


BRMI_EXPORTS = ["brmi_abi_version", "brmi_default_config", "brmi_create", "brmi_declare", "brmi_set_scene", "brmi_setup", "brmi_set_band",
                "brmi_update", "brmi_execute", "brmi_execute_split", "brmi_destroy", "brmi_last_error", "brmi_clear_visibility", "brmi_cull",
                "brmi_raster", "brmi_depth_copy", "brmi_build_hzb", "brmi_invalidate_hzb", "brmi_set_history_source", "brmi_gbuffer", "brmi_light_clustering",
                "brmi_shade", "brmi_set_shade_slabs", "brmi_read_counters", "brmi_stage_times", "brmi_set_timed_stages", "brmi_algorithmic_bytes", "brmi_algorithmic_bytes_launched", "brmi_debug_arith", "brmi_debug_arith_in_range", "brmi_debug_read_bin_records", "brmi_debug_wide_triangles", "brmi_debug_lean_clusters", "brmi_debug_raster_shape", "brmi_debug_read_lean_queue", "brmi_debug_read_held", "brmi_debug_read_draw_list",
                "brmi_streaming_scratch_bytes", "brmi_set_streaming", "brmi_streaming_feedback", "brmi_set_sampler_anisotropy", "brmi_debug_sample_grad",
                "brmi_abi_minor", "brmi_debug_view_bytes", "brmi_set_debug_view", "brmi_debug_view",
                "brmi_set_environment", "brmi_debug_ibl_lookup", "brmi_debug_ibl",
                "brmi_skybox", "brmi_env_convert", "brmi_env_project_sh", "brmi_env_prefilter", "brmi_env_build_bytes", "brmi_debug_env_lookup",
                "brmi_gtao_default_settings", "brmi_gtao_get_layout", "brmi_set_gtao", "brmi_gtao_prefilter", "brmi_gtao_main", "brmi_gtao_denoise",
                "brmi_texmips_bytes", "brmi_texmips_build", "brmi_texmips_build_alpha",
                "brmi_display_default_settings", "brmi_display_get_layout", "brmi_set_display", "brmi_display_exposure", "brmi_display_bloom", "brmi_display_resolve", "brmi_debug_display_bloom_pass", "brmi_debug_display_histogram",
                "brmi_set_shadows", "brmi_shadow_capture", "brmi_debug_shadow",
                "brmi_temporal_default_settings", "brmi_temporal_get_layout", "brmi_set_temporal", "brmi_temporal_resolve", "brmi_temporal_reset", "brmi_temporal_state",
                "brmi_debug_temporal_resolve"]


def brmi_lib():
    """libbrmi.so: HIP kernels + C ABI.  Fails loudly when the extension has not been built."""
    global _brmi_lib
    if _brmi_lib is None:
        # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7 / libhsa-runtime64 and owns
        # the device memory we are handed, so it must be loaded first; libbrmi.so's NEEDED libamdhip64.so.7
        # then resolves (by SONAME) to the copy already mapped instead of pulling in /opt/rocm's.
        import torch  # noqa: F401
        path = os.environ.get("BRMI_LIB_PATH") or os.path.join(LIB_DIR, "libbrmi.so")   # override: A/B builds of the same ABI
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: the HIP extension must be built (make hip); there is no CPU fallback")
        lib = C.CDLL(path)
        lib.brmi_abi_version.restype = u32
        lib.brmi_default_config.argtypes = [C.POINTER(Config), u32, u32]
        lib.brmi_default_config.restype = None
        lib.brmi_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
        lib.brmi_declare.argtypes = [vp, DECLARE_CB, vp]
        lib.brmi_set_scene.argtypes = [vp, C.POINTER(SceneBuffers)]
        lib.brmi_setup.argtypes = [vp, C.POINTER(ResourceBinding), u32, vp]
        lib.brmi_update.argtypes = [vp, C.POINTER(FrameUpdate), vp]
        lib.brmi_execute.argtypes = [vp, vp]
        lib.brmi_execute_split.argtypes = [vp, vp, vp]
        lib.brmi_destroy.argtypes = [vp]
        lib.brmi_destroy.restype = None
        lib.brmi_last_error.argtypes = [vp]
        lib.brmi_last_error.restype = C.c_char_p
        for n in ("brmi_clear_visibility", "brmi_depth_copy", "brmi_build_hzb", "brmi_gbuffer", "brmi_light_clustering", "brmi_shade"):
            getattr(lib, n).argtypes = [vp, vp]
        lib.brmi_invalidate_hzb.argtypes = [vp]
        lib.brmi_set_history_source.argtypes = [vp, vp]
        lib.brmi_set_shade_slabs.argtypes = [vp, u32, vp, vp]
        lib.brmi_cull.argtypes = [vp, u32, vp]
        lib.brmi_raster.argtypes = [vp, u32, vp]
        lib.brmi_read_counters.argtypes = [vp, C.POINTER(Counters), vp]
        lib.brmi_stage_times.argtypes = [vp, C.POINTER(f32)]
        lib.brmi_set_timed_stages.argtypes = [vp, u32]
        lib.brmi_algorithmic_bytes.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        lib.brmi_algorithmic_bytes_launched.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        lib.brmi_debug_arith.argtypes = [vp, vp, vp, vp, vp, u32, vp]
        lib.brmi_debug_arith_in_range.argtypes = [vp, vp, vp, vp, u32, vp]
        lib.brmi_streaming_scratch_bytes.argtypes = [u32]
        lib.brmi_streaming_scratch_bytes.restype = u64
        lib.brmi_set_streaming.argtypes = [vp, C.POINTER(StreamingBuffers)]
        lib.brmi_streaming_feedback.argtypes = [vp, vp]
        if hasattr(lib, "brmi_set_sampler_anisotropy"):      # (absent from an older build of the same ABI loaded through BRMI_LIB_PATH for an A/B run)
            lib.brmi_set_sampler_anisotropy.argtypes = [vp, vp, u32]
            lib.brmi_debug_sample_grad.argtypes = [C.POINTER(SceneBuffers), vp, u32, u32, u32, vp, vp, vp, vp, u32, vp]
        if hasattr(lib, "brmi_set_debug_view"):
            lib.brmi_abi_minor.restype = u32
            lib.brmi_debug_view_bytes.argtypes = [u32, u32]
            lib.brmi_debug_view_bytes.restype = u64
            lib.brmi_set_debug_view.argtypes = [vp, C.POINTER(DebugViewBuffers)]
            lib.brmi_debug_view.argtypes = [vp, vp]
        if hasattr(lib, "brmi_set_environment"):
            lib.brmi_set_environment.argtypes = [vp, C.POINTER(EnvironmentBuffers)]
            lib.brmi_debug_ibl_lookup.argtypes = [C.POINTER(EnvironmentBuffers), u32, vp, vp, vp, u32, vp]
            lib.brmi_debug_ibl.argtypes = [vp, C.POINTER(EnvironmentBuffers), u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp]
        if hasattr(lib, "brmi_skybox"):
            lib.brmi_skybox.argtypes = [vp, vp]
            lib.brmi_env_convert.argtypes = [vp, vp, u32, u32, vp]
            lib.brmi_env_project_sh.argtypes = [vp, u32, vp, u32, u32, u32, vp]
            lib.brmi_env_prefilter.argtypes = [vp, vp, u32, u32, u32, vp]
            lib.brmi_env_build_bytes.argtypes = [u32, u32, C.POINTER(u64), C.POINTER(u64)]
            lib.brmi_env_build_bytes.restype = u64
            lib.brmi_debug_env_lookup.argtypes = [vp, u32, u32, vp, vp, vp, u32, vp]
        if hasattr(lib, "brmi_set_gtao"):
            lib.brmi_gtao_default_settings.argtypes = [C.POINTER(GtaoSettings)]
            lib.brmi_gtao_default_settings.restype = None
            lib.brmi_gtao_get_layout.argtypes = [u32, u32, C.POINTER(GtaoLayout)]
            lib.brmi_set_gtao.argtypes = [vp, C.POINTER(GtaoBuffers)]
            for n in ("brmi_gtao_prefilter", "brmi_gtao_main", "brmi_gtao_denoise"):
                getattr(lib, n).argtypes = [vp, vp]
        if hasattr(lib, "brmi_texmips_build"):
            lib.brmi_texmips_bytes.argtypes = [u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
            lib.brmi_texmips_bytes.restype = u64
            lib.brmi_texmips_build.argtypes = [C.POINTER(TextureDesc), vp, vp, u64, vp]
            lib.brmi_texmips_build_alpha.argtypes = [C.POINTER(TextureDesc), vp, vp, vp, vp]
        if hasattr(lib, "brmi_set_display"):
            lib.brmi_display_default_settings.argtypes = [C.POINTER(DisplaySettings)]
            lib.brmi_display_default_settings.restype = None
            lib.brmi_display_get_layout.argtypes = [u32, u32, C.POINTER(DisplayLayout)]
            lib.brmi_set_display.argtypes = [vp, C.POINTER(DisplayBuffers)]
            for n in ("brmi_display_exposure", "brmi_display_bloom", "brmi_display_resolve", "brmi_debug_display_histogram"):
                getattr(lib, n).argtypes = [vp, vp]
            lib.brmi_debug_display_bloom_pass.argtypes = [vp, u32, u32, vp]
        if hasattr(lib, "brmi_set_shadows"):
            lib.brmi_set_shadows.argtypes = [vp, C.POINTER(ShadowBuffers)]
            lib.brmi_shadow_capture.argtypes = [vp, f32, f32, C.POINTER(TextureDesc), vp]
            lib.brmi_debug_shadow.argtypes = [vp, u32, vp, vp, vp, u32, vp]
        if hasattr(lib, "brmi_set_temporal"):
            lib.brmi_temporal_default_settings.argtypes = [C.POINTER(TemporalSettings)]
            lib.brmi_temporal_default_settings.restype = None
            lib.brmi_temporal_get_layout.argtypes = [u32, u32, C.POINTER(TemporalLayout)]
            lib.brmi_set_temporal.argtypes = [vp, C.POINTER(TemporalBuffers)]
            lib.brmi_temporal_resolve.argtypes = [vp, vp]
            lib.brmi_temporal_reset.argtypes = [vp]
            lib.brmi_temporal_state.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
            lib.brmi_debug_temporal_resolve.argtypes = [u32, u32, vp, vp, vp, vp, vp, C.POINTER(TemporalSettings), vp]
        _brmi_lib = lib
    return _brmi_lib
