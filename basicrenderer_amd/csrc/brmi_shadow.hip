// brmi_shadow.hip -- shadow maps of spot and point lights: a light view's depth as the R32F map the shader samples (brmi_shadow_capture),
// and the two shadow functions alone for made-up receivers (brmi_debug_shadow).  The functions themselves: brmi_shadow.h.
//
// Reference: BR/shaders/Include/shadows.hlsli:416-464,934-950, BR/shaders/Include/utilities.hlsli:2807-2810, BR/src/Utilities/Utilities.cpp:1926-1933
// (the light projection: XMMatrixPerspectiveFovRH(.., nearPlane, farPlane), whose depth is far * (z - near) / (z * (far - near)) for a view depth z).
#include "brmi_device.h"
#include "brmi_internal.h"
#include "brmi_shadow.h"

namespace brmi {

// One lane per map texel, row-major: the store is contiguous per wave, the read gathers from the pass's 8x8 tiles (a wave's 64 texels of one row touch eight
// tiles, 32 B of each).  A pixel without geometry holds the depth surface's "empty" word, which is what the visibility clear left there (k_depth_copy).
__global__ void __launch_bounds__(256) k_shadow_capture(const float* depth, uint32_t W, uint32_t H, uint32_t tilesX, float zNear, float zFar, float* dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    const uint32_t x = i % W, y = i / W;
    const float z = depth[tiled_index(x, y, tilesX)];
    float d = 1.0f;
    if (as_u32(z) != BRMI_DEPTH_EMPTY_BITS) d = zFar * (z - zNear) / (z * (zFar - zNear));
    dst[i] = d;
}
int launch_shadow_capture(brmi_pass* p, float zNear, float zFar, const brmi_texture_desc& dst, hipStream_t s) {
    const uint32_t W = p->cfg.width, H = p->cfg.height;
    hipLaunchKernelGGL(k_shadow_capture, dim3((W * H + 255u) / 256u), dim3(256), 0, s, static_cast<const float*>(p->res[BRMI_RES_LINEAR_DEPTH]), W, H, p->tilesX, zNear, zFar,
                       reinterpret_cast<float*>(const_cast<uint8_t*>(dst.texels)));
    BRMI_LAUNCH_CHECK(p, "k_shadow_capture");
    return BRMI_OK;
}

ShadowBind shadow_bind_of(const brmi_pass* p) {
    ShadowBind b{};
    if (!p->shadows.on) return b;
    const brmi_shadow_buffers& s = p->shadows.b;
    b.records = p->wsPtr<ShadowRecord>(p->ws.shadowRecords); b.maps = s.maps; b.spotCameras = s.spotCameraIndices; b.pointCameras = s.pointCameraIndices;
    b.cameras = p->scene.cameras;
    b.mapCount = s.mapCount; b.spotCount = s.spotCount; b.pointCount = s.pointCount; b.cameraCount = p->scene.cameraCount;
    return b;
}

// brmi_debug_shadow: light_shadow as the shading kernels call it, one receiver per lane; the record is built from the light as k_frame_constants builds it
__global__ void __launch_bounds__(256) k_debug_shadow(ShadowBind sb, const brmi_light_info* light, const float* pos, const float* nrm, float* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ShadowRecord r = shadow_record_of(kconst(light));
    float shadow = 0.0f;
    if (r.kind != SHADOW_NONE)
        shadow = light_shadow(sb, r, f3{light->posWorldSpace[0], light->posWorldSpace[1], light->posWorldSpace[2]}, f3{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}, f3{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]});
    out[i] = shadow;
}
int launch_debug_shadow(brmi_pass* p, uint32_t lightIndex, const float* positionsWS, const float* normalsWS, float* outShadow, uint32_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_debug_shadow, dim3((n + 255u) / 256u), dim3(256), 0, s, shadow_bind_of(p), p->scene.lights + lightIndex, positionsWS, normalsWS, outShadow, n);
    BRMI_LAUNCH_CHECK(p, "k_debug_shadow");
    return BRMI_OK;
}

}  // namespace brmi
