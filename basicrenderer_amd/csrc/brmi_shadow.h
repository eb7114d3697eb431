// brmi_shadow.h -- calculateSpotShadow and calculatePointShadow (BR/shaders/Include/shadows.hlsli:416-464, :934-950) as device code, restated as written
// (DESIGN.md 4.15).  The shading kernels' shadowed instantiations (brmi_shade.h) and brmi_debug_shadow (brmi_shadow.hip) call the same two functions.
// Every operation is IEEE fp32 without contraction, divisions and square roots correctly rounded: the result is a decision (0 or 1), and both direction
// instantiations of the light loop take it from the same correctly rounded inputs.
#ifndef BRMI_SHADOW_H
#define BRMI_SHADOW_H
#include "brmi_device.h"
#include "brmi_internal.h"
#include "brmi_texture.h"

namespace brmi {

// The per-light record k_frame_constants builds (brmi_frame.hip), indexed like the shading pass's light records by the position in the active-light list.
// kind 0: the light casts no shadow (a directional light; shadowViewInfoIndex or shadowMapIndex -1) -- one scalar test in the light loop.
constexpr uint32_t SHADOW_NONE = 0u, SHADOW_SPOT = 1u, SHADOW_POINT = 2u;
struct ShadowRecord { uint32_t kind, map, view; float nearPlane, farPlane; float dir[3]; };      // 32 B; dir: light.dirWorldSpace as stored (the spot bias reads it unnormalised)
static_assert(sizeof(ShadowRecord) == 32, "one s_load_dwordx8");

// brmi_set_shadows' tables as the kernels take them; `cameras` is the CALLER's camera buffer (the frame snapshot holds the main camera alone)
struct ShadowBind {
    const ShadowRecord* records; const brmi_texture_desc* maps; const uint32_t* spotCameras; const uint32_t* pointCameras; const brmi_camera* cameras;
    uint32_t mapCount, spotCount, pointCount, cameraCount;
};

// unprojectDepth (utilities.hlsli:2807-2810)
BRMI_DEV float unproject_depth(float depth, float nearP, float farP) { return nearP * farP / (farP - depth * (farP - nearP)); }

// One R32F level as the lookup reads it; a descriptor without texels or size reads as the border value everywhere (never a fault on a table that disagrees with itself)
struct ShadowMap { const float* texels; int w, h; };
template <typename DescPtr>
BRMI_DEV ShadowMap shadow_map_of(DescPtr d) {
    ShadowMap m; m.texels = reinterpret_cast<const float*>(d->texels); m.w = (int)d->width; m.h = (int)d->height;
    if (m.texels == nullptr || m.w <= 0 || m.h <= 0) { m.texels = nullptr; m.w = 1; m.h = 1; }
    return m;
}
// SampleLevel(.., uv, 0) as a plain bilinear fetch: the software sampler's footprint (u * w - 0.5, fp32 weights, a + t * (b - a) along x then y).
// BORDER: a tap outside the map reads 1.0 (the default shadow sampler's opaque-white border); otherwise the tap is clamped to the level (the cube's edge rule).
template <bool BORDER>
BRMI_DEV float shadow_bilinear(const ShadowMap& m, float u, float v) {
    const float fx = u * (float)m.w - 0.5f, fy = v * (float)m.h - 0.5f;
    const float tx = fx - floorf(fx), ty = fy - floorf(fy);
    const int x0 = floor_to_int(fx), y0 = floor_to_int(fy), x1 = inc_sat(x0), y1 = inc_sat(y0);
    auto tap = [&](int x, int y) {
        if (m.texels == nullptr) return 1.0f;
        if (BORDER) { if (x < 0 || y < 0 || x >= m.w || y >= m.h) return 1.0f; }
        else { x = x < 0 ? 0 : (x > m.w - 1 ? m.w - 1 : x); y = y < 0 ? 0 : (y > m.h - 1 ? m.h - 1 : y); }
        return m.texels[(size_t)y * (size_t)m.w + (size_t)x];
    };
    const float c00 = tap(x0, y0), c10 = tap(x1, y0), c01 = tap(x0, y1), c11 = tap(x1, y1);
    const float a = c00 + tx * (c10 - c00), b = c01 + tx * (c11 - c01);
    return a + ty * (b - a);
}

// calculateSpotShadow.  The record is wave-uniform (scalar registers); through kconst() so are the descriptor and the light camera's viewProjection.
BRMI_DEV float spot_shadow(const ShadowBind& sb, uint32_t map, uint32_t view, float nearP, float farP, f3 lightDir, f3 posWS, f3 normal) {
    if (map >= sb.mapCount || view >= sb.spotCount) return 0.0f;
    const uint32_t cam = kconst(sb.spotCameras)[view];
    if (cam >= sb.cameraCount) return 0.0f;
    const auto* vp = kconst(&sb.cameras[cam].viewProjection[0][0]);
    m4 M;
#pragma unroll
    for (int i = 0; i < 4; i++) { M.m[i][0] = vp[4 * i]; M.m[i][1] = vp[4 * i + 1]; M.m[i][2] = vp[4 * i + 2]; M.m[i][3] = vp[4 * i + 3]; }
    const f4 clip = mul_point(posWS, M);
    float u = clip.x / clip.w, v = clip.y / clip.w;
    u = u * 0.5f + 0.5f; v = v * 0.5f + 0.5f;
    v = 1.0f - v;
    const ShadowMap m = shadow_map_of(kconst(sb.maps + map));
    const float closestDepth = unproject_depth(shadow_bilinear<true>(m, u, v), nearP, farP);
    const float currentDepth = clip.z;                                 // clip-space z, NOT divided by w: as written
    const float bias = max2(0.0005f, 0.01f * (1.0f - dot3(normal, lightDir)));
    return currentDepth - bias > closestDepth ? 1.0f : 0.0f;
}

// calculatePointShadow.  The cube lookup takes the face, the texel addresses and the edge rule of the environment cube (cube_face_uv, clamp inside the face);
// the light camera is chosen by the shader's own `==` chain on maxDir, which is not the lookup's face rule and is restated separately.
BRMI_DEV float point_shadow(const ShadowBind& sb, uint32_t map, uint32_t view, float nearP, float farP, f3 lightPos, f3 posWS, f3 normal) {
    if (map + 5u >= sb.mapCount || map + 5u < map || view >= sb.pointCount) return 0.0f;
    f3 lightToFrag = posWS - lightPos;
    lightToFrag.z = -lightToFrag.z;
    const f3 worldDir = normalize3_q(lightToFrag);
    const CubeCoord c = cube_face_uv(worldDir);
    const ShadowMap m = shadow_map_of(sb.maps + map + c.face);
    const float depthSample = shadow_bilinear<false>(m, c.uv.x, c.uv.y);
    if (depthSample == 1.0f) return 0.0f;
    uint32_t faceIndex = 0u;
    const float maxDir = max2(max2(fabsf(worldDir.x), fabsf(worldDir.y)), fabsf(worldDir.z));
    if (worldDir.x == maxDir) faceIndex = 0u;
    else if (worldDir.x == -maxDir) faceIndex = 1u;
    else if (worldDir.y == maxDir) faceIndex = 2u;
    else if (worldDir.y == -maxDir) faceIndex = 3u;
    else if (worldDir.z == maxDir) faceIndex = 4u;
    else if (worldDir.z == -maxDir) faceIndex = 5u;
    const uint32_t cam = sb.pointCameras[view * 6u + faceIndex];
    if (cam >= sb.cameraCount) return 0.0f;
    const float closestDepth = unproject_depth(depthSample, nearP, farP);
    const f4 clip = mul_point(posWS, as_m4(sb.cameras[cam].viewProjection));
    const float lightSpaceDepth = clip.z;
    const float bias = max2(0.0005f, 0.02f * (1.0f - dot3(normal, worldDir)));
    return lightSpaceDepth - bias > closestDepth ? 1.0f : 0.0f;
}

// the light loop's `switch (light.type)` for a record whose kind is not SHADOW_NONE
BRMI_DEV float light_shadow(const ShadowBind& sb, const ShadowRecord& r, f3 lightPos, f3 posWS, f3 normal) {
    if (r.kind == SHADOW_SPOT) return spot_shadow(sb, r.map, r.view, r.nearPlane, r.farPlane, f3{r.dir[0], r.dir[1], r.dir[2]}, posWS, normal);
    return point_shadow(sb, r.map, r.view, r.nearPlane, r.farPlane, lightPos, posWS, normal);
}

// what k_frame_constants stores for light `l` (and brmi_debug_shadow builds for the light it is asked about)
template <typename LightPtr>
BRMI_DEV ShadowRecord shadow_record_of(LightPtr l) {
    ShadowRecord r;
    const bool casts = (l->type == BRMI_LIGHT_SPOT || l->type == BRMI_LIGHT_POINT) && l->shadowViewInfoIndex != -1 && l->shadowMapIndex != -1;
    r.kind = !casts ? SHADOW_NONE : (l->type == BRMI_LIGHT_SPOT ? SHADOW_SPOT : SHADOW_POINT);
    r.map = (uint32_t)l->shadowMapIndex; r.view = (uint32_t)l->shadowViewInfoIndex;
    r.nearPlane = l->nearPlane; r.farPlane = l->farPlane;
    r.dir[0] = l->dirWorldSpace[0]; r.dir[1] = l->dirWorldSpace[1]; r.dir[2] = l->dirWorldSpace[2];
    return r;
}

ShadowBind shadow_bind_of(const brmi_pass* p);      // host (brmi_shadow.hip): brmi_set_shadows' tables, all null / zero without a binding

}  // namespace brmi
#endif
