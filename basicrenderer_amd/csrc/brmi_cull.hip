// brmi_cull.hip -- hierarchical culling (K1-K3) for gfx950.
//
// What it computes is the reference's chain
//   PureComputeObjectCullCS / PureComputeTraverseFrontierCS   BR/shaders/ClusterLOD/computeCulling.hlsl:103-531
//   ClusterCullBody                                           BR/shaders/ClusterLOD/workGraphCulling.hlsl:2398-3330
// but not how the reference schedules it.  MI355X-first differences:
//   * HIP has no ExecuteIndirect, and a dependent chain of tiny dispatches is latency-bound
//     (SURVEY.md 8a-2).  The default path walks each instance's BVH inside ONE launch with the
//     frontier in LDS (k_cull_hierarchy: one wave64 per draw / replayed node).  Hierarchies whose
//     widest level exceeds the LDS frontier fall back to one fixed-size grid-stride launch per
//     level that reads its record count from HBM (k_cull_instances / k_traverse); either way the
//     chain is a static launch sequence with no host round trip.
//   * The reference appends survivors with wave ballots into one buffer, so the cluster index
//     that ends up in the visibility key depends on atomic ordering.  Here survivors set one bit
//     in a per-(instance, segment, meshlet) bitmask, a popcount scan ranks the bits, and a scatter
//     places each survivor at its rank: the visible-cluster list is identical run to run
//     (canonical order: instance, segment, meshlet) with one atomic per wave, not per survivor.
//   * Frontier / bucket appends are wave-aggregated (one atomic per wave64).
#include <type_traits>
#include "brmi_device.h"
#include "brmi_internal.h"
#include "brmi_lightgrid.h"
#include "brmi_texture.h"

namespace brmi {

struct CullArgs {
    brmi_scene_buffers sc;
    uint32_t* counters;
    const uint32_t* instanceBitBase;
    const uint32_t* segPrefix;
    uint32_t recordCapacity, visibleCapacity, factor, phase;
    // occlusion culling: phase 1 tests against the previous frame's chain with the previous transforms and appends what it
    // rejects to the replay buffers; phase 2 re-tests those against the chain of the depth phase 1 just rasterised
    uint32_t occlusion;
    uint32_t frontier0Counter, bucketCounter;   // counter words of the level-0 frontier and of the bucket array in use
    NodeRecord* replayNodes; BucketRecord* replayBuckets;
    HzbDesc hzb;
    // multi-GPU row band: two view-space planes through the eye bounding the band (1 = active)
    uint32_t bandActive; float bandTop[3], bandBottom[3];
    const float4* bandPlanes;        // the same two planes in memory (frameConst[3]): what the instance / node tests read
    StripeMap stripes;      // interleaved partition: ownership test of the cluster cull
    // mixed traversal: meshes whose widest BVH level fits the LDS frontier are walked by k_cull_hierarchy (one wave per instance, one launch),
    // the few wider ones by the level-per-launch kernels (all lanes of the chip on one level); the latter skip instances narrower than this
    const uint32_t* meshLevelWidth; uint32_t levelKernelsWidthLo;
    const FlatNode* flatNodes; const FlatLeaf* flatLeaves; const InstanceWalk* instanceWalk;     // flat traversal of small hierarchies (brmi_internal.h)
    uint32_t* feedback;                  // host-mapped words (brmi_pass::ensureFeedback) or null: word 2 = phase 1's bucket records (the host sizes the next frames' launches by it)
    uint32_t wideFlat;                   // phase 1: hierarchies of 257 .. 8192 nodes are k_cull_flat_wide's (the walk skips them)
    uint32_t packedFlat;                 // phase 1: the launch's first ceil(draws / 8) waves take eight draws each (hierarchies of <= 8 nodes)
};

BRMI_DEV f3 to_view_space(f3 c, const m4& model, const m4& view) { return xyz(mul_vm(mul_point(c, model), view)); }

BRMI_DEV bool sphere_outside_frustum(f3 c, float r, const float (*planes)[4]) {
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const float d = dot3(f3{planes[i][0], planes[i][1], planes[i][2]}, c) + planes[i][3];
        if (d < -r) return true;
    }
    return false;
}

BRMI_DEV float projected_error(f3 worldCenter, float worldRadius, float errMesh, float errScale, f3 camPos, float zNear, bool ortho) {
    const float wsErr = errMesh * errScale;
    if (ortho) return wsErr;
    const float dist = length3(worldCenter - camPos);
    const float denom = max2(dist - worldRadius, zNear);
    return wsErr / denom;
}

BRMI_DEV bool refined_child_suppresses(const brmi_scene_buffers& sc, uint32_t groupsBase, uint32_t childLocal, bool hasChild, const m4& model, float scale,
                                       f3 camPos, float zNear, float threshold, bool ortho) {
    if (!hasChild) return false;
    const brmi_lod_group* g = sc.lodGroups + (groupsBase + childLocal);
    const f3 c = xyz(mul_point(f3{g->centerAndRadius[0], g->centerAndRadius[1], g->centerAndRadius[2]}, model));
    const float r = g->centerAndRadius[3] * scale;
    const float eod = projected_error(c, r, g->maxParentError, scale, camPos, zNear, ortho);
    return !(eod < threshold);   // resident: static frame
}

// ---- residency-aware cut + streaming feedback (brmi_set_streaming; CLodGroupIsResident / CLodTouchAndRequestGroupResident, workGraphCulling.hlsl:1543-1629) ----
// The traversal kernels are compiled twice (brmi_cull_traversal.h): under their own names every group is resident (the code above, unchanged), as
// `..._streaming` they take a StreamArgs and follow the rule "... and the refined child group is resident".  The reference appends one record per touching thread to two lists and sorts; here a group has ONE bit
// ("touched") and ONE 64-bit word (the best request: bit 63 | priority16 << 32 | ~instanceIndex, kept with an atomic max, so the highest priority wins and
// among equals the lowest instance) in the caller's scratch, and brmi_streaming_feedback compacts and orders them.  Both are looked at before they are
// written: after a group's first touch of a frame the common case is one load and no atomic.
BRMI_DEV float refined_child_eod(const brmi_scene_buffers& sc, uint32_t childGlobal, const m4& model, float scale, f3 camPos, float zNear, bool ortho) {
    const brmi_lod_group* g = sc.lodGroups + childGlobal;
    const f3 c = xyz(mul_point(f3{g->centerAndRadius[0], g->centerAndRadius[1], g->centerAndRadius[2]}, model));
    return projected_error(c, g->centerAndRadius[3] * scale, g->maxParentError, scale, camPos, zNear, ortho);
}
BRMI_DEV bool stream_resident(const StreamArgs& st, uint32_t group) {
    return group < st.activeGroupScanCount && ((st.nonResidentBits[group >> 5] >> (group & 31u)) & 1u) == 0u;      // (activeGroupScanCount <= the group count: brmi_set_streaming)
}
// CLodTouchAndRequestGroupResident: marks the group touched, asks for it when it is not resident (never beyond activeGroupScanCount); true = resident
BRMI_DEV bool stream_touch(const StreamArgs& st, uint32_t group, uint32_t instanceIndex, float errorOverDistance) {
    if (group >= st.groupCount) return false;
    const uint32_t bit = 1u << (group & 31u);
    if ((__hip_atomic_load(&st.touchedBits[group >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) == 0u) atomicOr(&st.touchedBits[group >> 5], bit);
    if (stream_resident(st, group)) return true;
    if (group < st.activeGroupScanCount) {
        const unsigned long long key = (1ull << 63) | ((unsigned long long)stream_priority16(errorOverDistance) << 32) | (unsigned long long)(~instanceIndex);
        if (__hip_atomic_load(&st.requestKeys[group], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(&st.requestKeys[group], key);
    }
    return false;
}
// A leaf of the flat tables that turned out to be reached (its verdict was taken before that was known, from loads alone): the touches of
// the leaf preparation and of the refined-child test (workGraphCulling.hlsl:1631-1783), with the arithmetic the verdict used.
BRMI_DEV void flat_leaf_touch(const StreamArgs& st, const FlatNode& fn, const FlatLeaf& fl, uint32_t instIndex, const m4& model, float scale, f3 camPos, float zNear, float threshold, bool ortho) {
    const f3 gc = xyz(mul_point(f3{fl.group[0], fl.group[1], fl.group[2]}, model));
    const float eod = projected_error(gc, fl.group[3] * scale, fn.maxQuadricError, scale, camPos, zNear, ortho);
    if (!(eod >= threshold)) return;
    stream_touch(st, fl.ownerGlobal, instIndex, eod);
    if ((fn.info >> 1) & 1u) {
        const f3 cc = xyz(mul_point(f3{fl.child[0], fl.child[1], fl.child[2]}, model));
        const float ce = projected_error(cc, fl.child[3] * scale, fl.childParentError, scale, camPos, zNear, ortho);
        if (!(ce < threshold)) stream_touch(st, fl.childGlobal, instIndex, eod);
    }
}

// ceil(log2(x)) clamped to [0, maxMip], evaluated on the float's bits (the oracle's definition: stable next to powers of two)
BRMI_DEV uint32_t ceil_log2_clamped(float x, uint32_t maxMip) {
    if (!(x > 1.0f)) return 0u;
    const uint32_t u = __float_as_uint(x);
    const uint32_t m = ((u >> 23) & 0xFFu) - 127u + ((u & 0x7FFFFFu) ? 1u : 0u);
    return m < maxMip ? m : maxMip;
}

BRMI_DEV float hzb_load(const HzbDesc& h, uint32_t mip, uint32_t x, uint32_t y, uint32_t mipW) {
    if (mip == 0u) return (x < h.width && y >= h.rowLo && y < h.rowHi) ? h.depth[tiled_index(x, y, h.tilesX)] : __uint_as_float(BRMI_DEPTH_EMPTY_BITS);
    return h.mips[h.mipOffset[mip] + (size_t)y * mipW + x];
}

// sphere_screen_extents (Misc/sphereScreenExtents.hlsli:14-31) + OcclusionCullingPerspectiveTexture2D
// (occlusionCulling.hlsli:165-212): screen rectangle of the sphere -> mip whose texels cover it -> four point loads.
BRMI_DEV bool occlusion_culled(const HzbDesc& hzb, const brmi_camera* cam, float p00, float p11, f3 centerVS, float sphereDepth, float radius) {
    const float viewW = (float)cam->depthResX, viewH = (float)cam->depthResY;
    const float px = centerVS.x, py = -centerVS.y, pz = centerVS.z;
    const float rad2 = radius * radius, d = pz * radius;
    const float hv = sqrtf(px * px + pz * pz - rad2);
    const float ha = px * hv, hb = px * radius, hc = pz * hv;
    float L = (ha - d) * p00 / (hc + hb);
    float R = (ha + d) * p00 / (hc - hb);
    const float vv = sqrtf(py * py + pz * pz - rad2);
    const float va = py * vv, vb = py * radius, vc = pz * vv;
    const float B = (va - d) * p11 / (vc + vb);
    const float T = (va + d) * p11 / (vc - vb);
    L = -L; R = -R;
    const float u0 = sat(L * 0.5f + 0.5f), v0 = sat(T * -0.5f + 0.5f), u1 = sat(R * 0.5f + 0.5f), v1 = sat(B * -0.5f + 0.5f);
    const float ax0 = u0 * viewW, ay0 = v0 * viewH, ax1 = u1 * viewW, ay1 = v1 * viewH;
    const float ex = ax1 - ax0, ey = ay1 - ay0;
    const uint32_t mip = ceil_log2_clamped(max2(ex, ey), cam->numDepthMips - 1u);
    const float sx = cam->UVScaleToNextPowerOf2[0], sy = cam->UVScaleToNextPowerOf2[1];
    const float pu0 = u0 * sx, pv0 = v0 * sy, pu1 = u1 * sx, pv1 = v1 * sy;
    const float ssx = max2(sx, 1e-6f), ssy = max2(sy, 1e-6f);
    uint32_t hzbW = (uint32_t)rintf(viewW / ssx), hzbH = (uint32_t)rintf(viewH / ssy);
    hzbW = max(hzbW, 1u); hzbH = max(hzbH, 1u);
    const uint32_t mw = max(hzbW >> mip, 1u), mh = max(hzbH >> mip, 1u);
    uint32_t x0 = min((uint32_t)floorf(pu0 * (float)mw), mw - 1u), y0 = min((uint32_t)floorf(pv0 * (float)mh), mh - 1u);
    uint32_t x1 = min((uint32_t)floorf(pu1 * (float)mw), mw - 1u), y1 = min((uint32_t)floorf(pv1 * (float)mh), mh - 1u);
    if (stripe_on(hzb.stripes)) {
        // Interleaved partition (no counterpart in the reference): the chain is built from this GPU's compact depth surface, so the rectangle's
        // frame rows are mapped onto the surface rows this GPU owns among them -- consecutive surface rows -- and the mip is chosen from THAT
        // extent; a rectangle of extent <= 2^mip spans at most two texels per axis, so the four corner texels cover it.  A rectangle that
        // holds none of this GPU's rows says nothing here (the ownership test of the cluster cull drops such clusters for good).
        const uint32_t H = hzb.stripes.fullHeight;
        const uint32_t r0 = min((uint32_t)floorf(ay0), H - 1u), r1 = min((uint32_t)floorf(ay1), H - 1u);
        const uint32_t f = stripe_first_owned(hzb.stripes, r0), l = stripe_last_owned(hzb.stripes, r1);
        if (l == 0xFFFFFFFFu || f > l) return false;
        const uint32_t vy0 = stripe_vrow(hzb.stripes, f), vy1 = stripe_vrow(hzb.stripes, l);
        const uint32_t smip = ceil_log2_clamped(max2(fabsf(ex) + 1.0f, (float)(vy1 - vy0 + 1u)), hzb.mipCount - 1u);      // (|ex|: the reference's horizontal extents come out swapped; here the test has to be conservative)
        const uint32_t smw = max(hzb.paddedW >> smip, 1u), smh = max(hzb.paddedH >> smip, 1u);
        const uint32_t px0 = min((uint32_t)floorf(min2(ax0, ax1)), hzb.width - 1u), px1 = min((uint32_t)floorf(max2(ax0, ax1)), hzb.width - 1u);
        x0 = min(px0 >> smip, smw - 1u); x1 = min(px1 >> smip, smw - 1u); y0 = min(vy0 >> smip, smh - 1u); y1 = min(vy1 >> smip, smh - 1u);
        const float e0 = hzb_load(hzb, smip, x0, y0, smw), e1 = hzb_load(hzb, smip, x1, y0, smw), e2 = hzb_load(hzb, smip, x1, y1, smw), e3 = hzb_load(hzb, smip, x0, y1, smw);
        return max2(max2(e0, e1), max2(e2, e3)) < sphereDepth - radius;
    }
    if (mip >= hzb.mipCount) return false;
    const float d0 = hzb_load(hzb, mip, x0, y0, mw), d1 = hzb_load(hzb, mip, x1, y0, mw), d2 = hzb_load(hzb, mip, x1, y1, mw), d3 = hzb_load(hzb, mip, x0, y1, mw);
    const float mx = max2(max2(d0, d1), max2(d2, d3));
    return mx < sphereDepth - radius;
}

// phase 1: previous frame's transforms (the chain is the previous frame's depth); phase 2 / replay: current ones
BRMI_DEV bool occlusion_test(const CullArgs& a, const brmi_camera* cam, bool replay, f3 localCenter, float localRadius, f3 currentVS, float currentRadius,
                             const brmi_per_object* obj) {
    if (replay) return occlusion_culled(a.hzb, cam, cam->projection[0][0], cam->projection[1][1], currentVS, -currentVS.z, currentRadius);
    const m4 prevModel = load_m4(&obj->prevModel[0][0]);
    const f3 pc = to_view_space(localCenter, prevModel, load_m4(&cam->prevView[0][0]));
    return occlusion_culled(a.hzb, cam, cam->prevUnjitteredProjection[0][0], cam->prevUnjitteredProjection[1][1], pc, -pc.z, localRadius * max_axis_scale(prevModel));
}

// phase 1's test with the previous model matrix already in registers (the flat traversal requests it together with the current one: behind the
// node tests it was a memory round trip of its own in front of the depth chain's)
BRMI_DEV bool occlusion_test_prev(const CullArgs& a, const brmi_camera* cam, f3 localCenter, float localRadius, const m4& prevModel) {
    const f3 pc = to_view_space(localCenter, prevModel, load_m4(&cam->prevView[0][0]));
    return occlusion_culled(a.hzb, cam, cam->prevUnjitteredProjection[0][0], cam->prevUnjitteredProjection[1][1], pc, -pc.z, localRadius * max_axis_scale(prevModel));
}

// Interleaved partition: does the sphere's screen rectangle (the vertical extents of sphere_screen_extents, two rows of slack) hold a row
// this GPU owns?  Spheres that reach the near plane are kept (the extents are not defined there).
BRMI_DEV bool stripe_rejects(const StripeMap& m, const brmi_camera* cam, f3 centerVS, float radius) {
    const float pz = centerVS.z;
    if (!(-pz - radius > cam->zNear)) return false;
    const float py = -centerVS.y, p11 = cam->projection[1][1];
    const float rad2 = radius * radius, d = pz * radius;
    const float vv = sqrtf(py * py + pz * pz - rad2);
    const float va = py * vv, vb = py * radius, vc = pz * vv;
    const float B = (va - d) * p11 / (vc + vb), T = (va + d) * p11 / (vc - vb);
    const float v0 = sat(T * -0.5f + 0.5f), v1 = sat(B * -0.5f + 0.5f);
    if (!(v0 <= v1)) return false;
    const float H = (float)m.fullHeight;
    const int r0 = max(to_int_sat(floorf(v0 * H)) - 2, 0), r1 = min(to_int_sat(floorf(v1 * H)) + 2, (int)m.fullHeight - 1);
    return stripe_first_owned(m, (uint32_t)r0) > (uint32_t)r1;
}

// Frustum test of an instance's or a hierarchy node's sphere, and -- interleaved partition, round 4 -- the ownership test on top of it: a sphere whose
// screen rows (two rows of slack) hold none of this GPU's rows is not descended.  The cluster cull drops exactly such meshlets anyway
// (stripe_rejects on the meshlet's own sphere, inside the node's); before this every rank walked every node and tested every meshlet of the
// N-times-taller frame, which is where the render-side 0.78 of profiles/r03_rank_balance.md came from.  Dropped, not replayed.
// Round 6: the same for the contiguous band (brmi_config::bandY0 / bandY1, brmi_set_band) -- its two view-space planes through the eye, which the cluster cull already tested
// per meshlet: every rank of the 8-GPU San-Miguel-class frame visited all 37,600 nodes and tested 40 k meshlets for bands that show 24 .. 27 k clusters.
BRMI_DEV bool sphere_culled(const CullArgs& a, const brmi_camera* cam, f3 c, float r) {
    if (sphere_outside_frustum(c, r, cam->clippingPlanes)) return true;
    if (a.bandActive) {      // (the planes from memory, like the camera's: brmi_frame.hip)
        const float4 top = a.bandPlanes[0], bottom = a.bandPlanes[1];
        if ((top.x * c.x + top.y * c.y) + top.z * c.z < -r || (bottom.x * c.x + bottom.y * c.y) + bottom.z * c.z < -r) return true;
    }
    return stripe_on(a.stripes) && stripe_rejects(a.stripes, cam, c, r);
}

// K1 -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cull_instances(CullArgs a, NodeRecord* frontier0) {
    const brmi_scene_buffers& sc = a.sc;
    const uint32_t viewId = sc.perFrame->mainCameraIndex;
    const brmi_camera* cam = sc.cameras + viewId;
    const m4 view = load_m4(&cam->view[0][0]);
    for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < ((sc.activeDrawCount + 63u) & ~63u); d += gridDim.x * blockDim.x) {
        bool visible = false;
        uint32_t ii = 0, root = 0;
        if (d < sc.activeDrawCount && (a.levelKernelsWidthLo == 0u || a.meshLevelWidth[sc.clodOffsets[sc.activeDraws[d]].clodMeshMetadataIndex] >= a.levelKernelsWidthLo)) {
            ii = sc.activeDraws[d];
            const brmi_per_mesh_instance inst = sc.perMeshInstance[ii];
            const m4 model = load_m4(&sc.perObject[inst.perObjectBufferIndex].model[0][0]);
            const f3 c = to_view_space(f3{inst.boundingSphere[0], inst.boundingSphere[1], inst.boundingSphere[2]}, model, view);
            const float r = inst.boundingSphere[3] * max_axis_scale(model);
            const bool bad = isnan(c.x) || isnan(c.y) || isnan(c.z) || isinf(c.x) || isinf(c.y) || isinf(c.z) || isnan(r) || isinf(r);
            visible = !bad && !sphere_culled(a, cam, c, r);
            root = sc.meshMetadata[sc.clodOffsets[ii].clodMeshMetadataIndex].rootNode;
            atomicAdd(&a.counters[CNT_INSTANCES_TESTED], 1u);
            if (visible) atomicAdd(&a.counters[CNT_INSTANCES_VISIBLE], 1u);
        }
        const uint32_t slot = wave_append(&a.counters[CNT_FRONTIER0], visible);
        if (visible) {
            if (slot < a.recordCapacity) frontier0[slot] = NodeRecord{ii, (1u << 30) | (root & 0x3FFFFFFFu)};
            else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
        }
    }
}

// K2, K1 + K2 in one launch, the flat evaluations and K3 live in brmi_cull_traversal.h, compiled twice: without and with the residency rule
#ifndef BRMI_HIER_STAGE_WIDE
#define BRMI_HIER_STAGE_WIDE 128
#endif
constexpr uint32_t HIER_CAP_MAX = 1024;   // widest BVH level the LDS frontier variants cover
struct NoSide {};
struct SideJobs { ulonglong2* vis2; uint64_t n2; uint32_t walkBlocks, clearBlocks; ClusterArgs lc; };
constexpr uint32_t FLAT_WIDE_MAX = 8192;
struct LcRide { uint32_t mainBlocks; ClusterArgs lc; };
struct ClearRide { uint32_t mainBlocks; ulonglong2* vis2; uint64_t n2; uint32_t clearBlocks; };

// ComputeSkinnedMeshletBounds (workGraphCulling.hlsl:1405-1467): the meshlet sphere moved by every bone the meshlet lists,
// merged pairwise into one enclosing sphere
BRMI_DEV float4 skinned_meshlet_bounds(const brmi_scene_buffers& sc, const brmi_meshlet_descriptor* desc, const brmi_page_header* hdr, const uint8_t* page, uint32_t slot, float4 staticBounds) {
    const uint32_t boneCount = desc->boneCount;
    if (slot == 0xFFFFFFFFu || boneCount == 0u || sc.skinningMatrices == nullptr) return staticBounds;
    const uint32_t* boneList = reinterpret_cast<const uint32_t*>(page + hdr->boneIndexStreamOffset + desc->boneListOffset * 4u);
    const f3 c0{staticBounds.x, staticBounds.y, staticBounds.z};
    f3 mc{0.0f, 0.0f, 0.0f}; float mr = 0.0f; bool init = false;
    for (uint32_t b = 0; b < boneCount; b++) {
        const m4 m = load_bone_skin_matrix(sc.skinningMatrices, slot, boneList[b]);
        const f3 tc = xyz(mul_point(c0, m));
        const float tr = staticBounds.w * max_axis_scale(m);
        if (!init) { mc = tc; mr = tr; init = true; continue; }
        const f3 delta = tc - mc;
        const float dist = length3(delta);
        if (dist + tr <= mr) continue;
        if (dist + mr <= tr) { mc = tc; mr = tr; continue; }
        const float newRadius = 0.5f * (dist + mr + tr);
        const float t = (newRadius - mr) / max2(dist, 1e-12f);
        mc = mc + delta * t;
        mr = newRadius;
    }
    if (!init) return staticBounds;
    return make_float4(mc.x, mc.y, mc.z, mr * (1.0f + 1e-5f));
}

#define BRMI_STREAMING_PASS 0
#include "brmi_cull_traversal.h"
#undef BRMI_STREAMING_PASS
#define BRMI_STREAMING_PASS 1
#include "brmi_cull_traversal.h"
#undef BRMI_STREAMING_PASS

// rank = exclusive popcount scan over the bitmask ----------------------------------------------
constexpr uint32_t SCAN_BLOCK_WORDS = 2048;   // words per workgroup (256 threads x 8)

// blockDirty: a block no survivor set a bit in sums to zero unread and needs no word prefixes (nobody asks for the rank of a bit that is not set): phase 2
// of a Zorah-class frame places a hundred clusters in a bitmask of 12.8 M words.
__global__ void __launch_bounds__(256) k_scan_reduce(const uint32_t* bitmask, uint32_t totalWords, uint32_t* blockSums, const uint8_t* blockDirty) {
    __shared__ uint32_t partial[4];
    if (blockDirty[blockIdx.x] == 0) { if (threadIdx.x == 0) blockSums[blockIdx.x] = 0u; return; }
    const uint32_t base = blockIdx.x * SCAN_BLOCK_WORDS;
    uint32_t s = 0;
    for (uint32_t i = threadIdx.x; i < SCAN_BLOCK_WORDS; i += 256) { const uint32_t w = base + i; if (w < totalWords) s += __popc(bitmask[w]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor((int)s, o);
    if ((threadIdx.x & 63u) == 0) partial[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) blockSums[blockIdx.x] = partial[0] + partial[1] + partial[2] + partial[3];
}

// single workgroup: exclusive scan of blockSums in place; total -> counters[outIndex] (clamped to capacity)
__global__ void __launch_bounds__(1024) k_scan_blocks(uint32_t* blockSums, uint32_t nBlocks, uint32_t* counters, uint32_t outIndex, uint32_t capacity, uint32_t usedIndex, uint32_t* hostFeedback) {
    __shared__ uint32_t waveTotals[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nBlocks; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nBlocks ? blockSums[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if ((threadIdx.x & 63u) >= (uint32_t)o) incl += t; }
        if ((threadIdx.x & 63u) == 63u) waveTotals[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t waveBase = 0;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) waveBase += waveTotals[w];
        const uint32_t c = carry;
        if (i < nBlocks) blockSums[i] = c + waveBase + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + waveBase + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t placed = min(carry, capacity - (usedIndex == 0xFFFFFFFFu ? 0u : min(counters[usedIndex], capacity)));
        counters[outIndex] = placed;
        if (hostFeedback) __hip_atomic_store(hostFeedback, placed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // (phase 2: the host's hint for the next frames)
    }
}

__global__ void __launch_bounds__(256) k_scan_words(const uint32_t* bitmask, uint32_t totalWords, const uint32_t* blockSums, uint32_t* wordPrefix, const uint8_t* blockDirty) {
    __shared__ uint32_t waveTotals[4];
    __shared__ uint32_t carry;
    if (blockDirty[blockIdx.x] == 0) return;
    if (threadIdx.x == 0) carry = blockSums[blockIdx.x];
    __syncthreads();
    const uint32_t base = blockIdx.x * SCAN_BLOCK_WORDS;
    for (uint32_t chunk = 0; chunk < SCAN_BLOCK_WORDS; chunk += 256) {
        const uint32_t w = base + chunk + threadIdx.x;
        const uint32_t v = w < totalWords ? __popc(bitmask[w]) : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if ((threadIdx.x & 63u) >= (uint32_t)o) incl += t; }
        if ((threadIdx.x & 63u) == 63u) waveTotals[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t waveBase = 0;
        for (uint32_t k = 0; k < (threadIdx.x >> 6); k++) waveBase += waveTotals[k];
        const uint32_t c = carry;
        if (w < totalWords) wordPrefix[w] = c + waveBase + incl - v;
        __syncthreads();
        if (threadIdx.x == 255) carry = c + waveBase + incl;
        __syncthreads();
    }
}

// The three kernels above as ONE launch for bitmasks of up to 64 blocks (131 k words: every benchmark frame has 6-10): a block counts its 2048
// words, publishes the sum with the launch's epoch in one 64-bit agent-scope store, waits for the sums of the blocks before it (all <= 64
// blocks are resident at once: 256 CUs), and scans its words from there; the last block writes the total.  Two launches less per culling
// phase -- with another frame's shading pass filling the chip every small launch of the geometry stream waits 5-15 us for its slots.
constexpr uint32_t SCAN_CHAIN_BLOCKS = 64;
__global__ void __launch_bounds__(256) k_scan_chained(const uint32_t* bitmask, uint32_t totalWords, unsigned long long* agg, uint32_t epoch, uint32_t* wordPrefix,
                                                     uint32_t* counters, uint32_t outIndex, uint32_t capacity, uint32_t usedIndex, uint32_t* hostFeedback) {
    __shared__ uint32_t waveTotals[4];
    __shared__ uint32_t blockPrefix, ticket;
    // the block's place in the chain is the order in which blocks START (a ticket), not blockIdx: a block only ever waits for blocks that are
    // running already, whatever order the dispatcher picks (agg[64] is the ticket word; the last block puts it back to zero)
    if (threadIdx.x == 0) ticket = (uint32_t)__hip_atomic_fetch_add(&agg[SCAN_CHAIN_BLOCKS], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint32_t block = ticket;
    const uint32_t base = block * SCAN_BLOCK_WORDS + threadIdx.x * 8u;       // eight consecutive words per thread
    uint32_t pc[8], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) { const uint32_t w = base + k; pc[k] = w < totalWords ? (uint32_t)__popc(bitmask[w]) : 0u; sum += pc[k]; }
    uint32_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if ((threadIdx.x & 63u) >= (uint32_t)o) incl += t; }
    if ((threadIdx.x & 63u) == 63u) waveTotals[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t waveBase = 0, blockSum = 0;
    for (uint32_t k = 0; k < 4u; k++) { if (k < (threadIdx.x >> 6)) waveBase += waveTotals[k]; blockSum += waveTotals[k]; }
    if (threadIdx.x == 0) __hip_atomic_store(&agg[block], ((unsigned long long)epoch << 32) | blockSum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x < 64u) {
        uint32_t mine = 0;
        if (threadIdx.x < block) {
            unsigned long long v;
            do { v = __hip_atomic_load(&agg[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while ((uint32_t)(v >> 32) != epoch);
            mine = (uint32_t)v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o);
        if (threadIdx.x == 0) blockPrefix = mine;
    }
    __syncthreads();
    uint32_t run = blockPrefix + waveBase + incl - sum;
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) { const uint32_t w = base + k; if (w < totalWords) wordPrefix[w] = run; run += pc[k]; }
    if (block == gridDim.x - 1u && threadIdx.x == 0) {
        __hip_atomic_store(&agg[SCAN_CHAIN_BLOCKS], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // every ticket of this launch has been taken
        const uint32_t placed = min(blockPrefix + blockSum, capacity - (usedIndex == 0xFFFFFFFFu ? 0u : min(counters[usedIndex], capacity)));
        counters[outIndex] = placed;
        if (hostFeedback) __hip_atomic_store(hostFeedback, placed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // (phase 2: the host's hint for the next frames)
    }
}

// Places every survivor at its rank.  Also accumulates the vertex / triangle totals of the clusters that will be
// rasterised (statistics for the algorithmic-byte count), one atomic per wave: a per-cluster atomic on three
// shared words would serialise the whole rasteriser (~90 same-address atomics per microsecond).
// LOCAL_RANK (survivor bitmasks of <= LOCAL_RANK_WORDS words: every BASELINE-class scene): no rank kernel runs before this one; every
// workgroup that has survivors to place scans the popcounts itself into LDS (a few thousand L2-resident words), workgroup 0 publishes the
// total.  One ~5 us launch less per culling phase.  Larger bitmasks take the three scan launches (a variant with one LDS prefix per group
// of words up to 2^17 words was measured on the dense frame's 25 k words: 55 us per phase against 27).
#ifndef BRMI_LOCAL_RANK_WORDS
#define BRMI_LOCAL_RANK_WORDS 8192
#endif
constexpr uint32_t LOCAL_RANK_WORDS = BRMI_LOCAL_RANK_WORDS;
struct LocalRank { uint32_t totalWords, outIndex, usedIndex; uint32_t* hostFeedback; };
// Round 6: the lists of a frame that holds clusters back (brmi_raster.hip).  drawList == nullptr: every cluster of the visible list is rasterised in list order, as before.
struct DrawLists {
    uint32_t* drawList; HeldRecord* held; uint32_t countAll;      // countAll: phase 2 of such a frame -- every placed cluster is drawn and counts
    // the prediction's inputs (phase 1): the chain the reference's test just read, the per-meshlet boxes, the per-object constants, the chain's size
    // (box_behind_chain, brmi_internal.h: the same question the re-test asks -- of the PREVIOUS frame's chain with the previous frame's matrices.  The reference's own
    // test asks it of the meshlet's SPHERE with four texels of a coarser mip, and lets through twice the clusters that own a pixel: profiles/r06_experiments.md --
    // a box's near corner is the surface's, a sphere's near point half a cluster in front of it.)
    const MeshletBox* boxes; const uint32_t* pageBoxBase; const float* objConst; uint32_t maxTexels; BoxViewport vp; HzbDesc hzb;
};
template <bool LOCAL_RANK, bool HOLD>      // HOLD: phase 1 of a frame that holds clusters back (the prediction and the two lists; the plain instantiations keep their registers)
__global__ void __launch_bounds__(256) k_scatter_visible(const TempVisible* temp, uint32_t* counters, uint32_t tempCountIndex, const uint32_t* bitmask,
                                                        const uint32_t* wordPrefix, uint4* visible, uint32_t baseIndexCounter, uint32_t capacity, uint32_t visibleCapacity,
                                                        brmi_scene_buffers sc, ClusterSetup* setup, uint32_t resolveCapacity, ClusterUv* clusterUv, LocalRank lr, DrawLists dl) {
    const uint8_t* const* slabs = sc.slabs;
    const uint32_t n = min(counters[tempCountIndex], visibleCapacity);
    const uint32_t base = baseIndexCounter == 0xFFFFFFFFu ? 0u : counters[baseIndexCounter];
    const uint32_t rounded = (n + 63u) & ~63u;
    __shared__ uint32_t prefixLds[LOCAL_RANK ? LOCAL_RANK_WORDS : 1];
    __shared__ uint32_t waveTotals[4];
    if (LOCAL_RANK) {
        if (blockIdx.x != 0u && blockIdx.x * blockDim.x >= rounded) return;       // nothing to place here (workgroup 0 always publishes the total)
        const uint32_t span = (lr.totalWords + 255u) / 256u;
        const uint32_t w0 = threadIdx.x * span, w1 = min(w0 + span, lr.totalWords);
        uint32_t sum = 0;
        for (uint32_t w = w0; w < w1; w++) sum += __popc(bitmask[w]);
        uint32_t incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if ((threadIdx.x & 63u) >= (uint32_t)o) incl += t; }
        if ((threadIdx.x & 63u) == 63u) waveTotals[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t waveBase = 0, all = 0;
        for (uint32_t w = 0; w < 4; w++) { if (w < (threadIdx.x >> 6)) waveBase += waveTotals[w]; all += waveTotals[w]; }
        uint32_t run = waveBase + incl - sum;
        for (uint32_t w = w0; w < w1; w++) { prefixLds[w] = run; run += __popc(bitmask[w]); }
        if (blockIdx.x == 0u && threadIdx.x == 0u) {
            const uint32_t placed = min(all, capacity - (lr.usedIndex == 0xFFFFFFFFu ? 0u : min(counters[lr.usedIndex], capacity)));
            counters[lr.outIndex] = placed;
            if (lr.hostFeedback) __hip_atomic_store(lr.hostFeedback, placed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __syncthreads();
    }
    // (statistics double as the reservation of the clusters' tables in the resolve arena.  Round 5: ONE atomic per workgroup -- vertices in the low,
    // triangles in the high half of one 64-bit word -- instead of three per wave on one cache line: a Zorah-class frame places 490 k clusters, and
    // 23 k same-line atomics at ~90 per microsecond were 250 us, the whole kernel.  The count of placed clusters is one thread's sum.)
    __shared__ unsigned long long blockBase;
    __shared__ uint32_t waveV[4], waveT[4], waveD[4], waveH[4], blockDraw, blockHeld;
    unsigned long long drawnVT = 0ull;      // this thread's share of the vertex | triangle << 32 sums of the clusters on the draw list
    if (blockIdx.x == 0u && threadIdx.x == 0u) { const uint32_t room = base < capacity ? capacity - base : 0u; atomicAdd(&counters[CNT_RASTER_CLUSTERS], min(n, room)); if (resolveCapacity == 0u && n != 0u) atomicOr(&counters[CNT_RESOLVE_SPILL], 1u); }
    const uint32_t rounded256 = (n + 255u) & ~255u;      // workgroup-uniform trip count (barriers inside)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < rounded256; i += gridDim.x * blockDim.x) {
        uint32_t verts = 0, tris = 0, placed = 0, dst = 0;
        TempVisible t{};
        const uint8_t* slab = nullptr; uint32_t pageOff = 0;
        const brmi_page_header* hdr = nullptr; const brmi_meshlet_descriptor* desc = nullptr;
        uint32_t held = 0u, boxIndex = 0xFFFFFFFFu, perObject = 0u;
        if (i < n) {
            t = temp[i];
            const uint32_t w = t.bit >> 5, b = t.bit & 31u;
            const uint32_t rank = (LOCAL_RANK ? prefixLds[w] : wordPrefix[w]) + __popc(bitmask[w] & ((1u << b) - 1u));
            dst = base + rank;
            if (dst < capacity) {
                visible[dst] = t.packed;
                slab = slabs[vc_slab(t.packed)];
                pageOff = vc_page_offset(t.packed);
                hdr = reinterpret_cast<const brmi_page_header*>(slab + pageOff);
                desc = reinterpret_cast<const brmi_meshlet_descriptor*>(slab + pageOff + hdr->descriptorOffset + vc_meshlet(t.packed) * 64u);
                verts = min((desc->bitsAndVertexCount >> 24) & 0xFFu, BRMI_MESHLET_MAX_VERTS);
                tris = min(desc->triangleCountAndRefinedGroup & 0xFFFFu, BRMI_MESHLET_MAX_TRIS);
                placed = 1;
                if (HOLD) {
                    // (round 6: the cluster is visible as far as the reference's tests go and has its place in the list; is it worth drawing FIRST?)
                    const brmi_per_mesh_instance inst = sc.perMeshInstance[vc_instance(t.packed)];
                    perObject = inst.perObjectBufferIndex;
                    const uint32_t boxBase = dl.pageBoxBase[(size_t)vc_slab(t.packed) * 1024u + (pageOff >> 18)];
                    if (boxBase != 0xFFFFFFFFu && (sc.perMesh[inst.perMeshBufferIndex].vertexFlags & BRMI_VERTEX_SKINNED) == 0u) {
                        boxIndex = boxBase + vc_meshlet(t.packed);
                        const MeshletBox bx = dl.boxes[boxIndex];
                        const float* oc = dl.objConst + (size_t)perObject * OBJ_CONST_FLOATS;
                        if (bx.valid && box_behind_chain(dl.hzb, bx, oc + 36, oc + 52, dl.vp, dl.maxTexels)) held = 1u;
                    }
                }
            }
        }
        uint32_t inclV = verts, inclT = tris;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)inclV, o), tt = (uint32_t)__shfl_up((int)inclT, o);
            if ((threadIdx.x & 63u) >= (uint32_t)o) { inclV += v; inclT += tt; }
        }
        // the draw list and the held records: slots per workgroup, like the arena's
        const bool isHeld = HOLD && placed != 0u && held != 0u, isDraw = HOLD && placed != 0u && !isHeld;
        const uint64_t drawM = __ballot(isDraw), heldM = __ballot(isHeld);
        __syncthreads();                                  // the previous round's base and wave sums have been read
        if ((threadIdx.x & 63u) == 63u) { waveV[threadIdx.x >> 6] = inclV; waveT[threadIdx.x >> 6] = inclT; waveD[threadIdx.x >> 6] = (uint32_t)__popcll(drawM); waveH[threadIdx.x >> 6] = (uint32_t)__popcll(heldM); }
        __syncthreads();
        if (threadIdx.x == 0u) {
            const unsigned long long totV = (unsigned long long)waveV[0] + waveV[1] + waveV[2] + waveV[3], totT = (unsigned long long)waveT[0] + waveT[1] + waveT[2] + waveT[3];
            blockBase = (totV | totT) ? atomicAdd(reinterpret_cast<unsigned long long*>(&counters[CNT_SUM_VERTS_LO]), totV | (totT << 32)) : 0ull;
        }
        if (HOLD && threadIdx.x == 64u) { const uint32_t tot = waveD[0] + waveD[1] + waveD[2] + waveD[3]; blockDraw = tot ? atomicAdd(&counters[CNT_DRAW1], tot) : 0u; }
        if (HOLD && threadIdx.x == 128u) { const uint32_t tot = waveH[0] + waveH[1] + waveH[2] + waveH[3]; blockHeld = tot ? atomicAdd(&counters[CNT_HELD1], tot) : 0u; }
        __syncthreads();
        if (dl.countAll && placed) drawnVT += (unsigned long long)verts | ((unsigned long long)tris << 32);
        if (isDraw || isHeld) {
            uint32_t slot = (isDraw ? blockDraw : blockHeld) + lane_rank(isDraw ? drawM : heldM);
            for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) slot += isDraw ? waveD[w] : waveH[w];
            if (isDraw) { dl.drawList[slot] = dst; drawnVT += (unsigned long long)verts | ((unsigned long long)tris << 32); }
            else dl.held[slot] = HeldRecord{dst, boxIndex, perObject, verts | (tris << 16)};
        }
        unsigned long long baseV = (uint32_t)blockBase, baseT = blockBase >> 32;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) { baseV += waveV[w]; baseT += waveT[w]; }
        if (placed) {
            // resolve the cluster for the rasteriser and the G-buffer pass
            const uint32_t instanceIndex = vc_instance(t.packed);
            const brmi_per_mesh_instance inst = sc.perMeshInstance[instanceIndex];
            const brmi_per_object* obj = sc.perObject + inst.perObjectBufferIndex;
            ClusterSetup cs;
            cs.posBase = slab + pageOff + hdr->positionBitstreamOffset + desc->positionBitOffset;
            cs.triBase = slab + pageOff + hdr->triangleStreamOffset + desc->triangleByteOffset;
            cs.nrmBase = slab + pageOff + hdr->normalArrayOffset + desc->vertexAttributeOffset * 4u;
            const brmi_per_mesh* pm = sc.perMesh + inst.perMeshBufferIndex;
            cs.counts = verts | (tris << 8) | ((hdr->compressedPositionQuantExp & 0xFFu) << 16) | (((obj->objectFlags & BRMI_OBJECT_FLAG_REVERSE_WINDING) != 0 ? 1u : 0u) << 24)
                      | ((pm->vertexFlags & BRMI_VERTEX_SKINNED) ? BRMI_CS_SKINNED : 0u) | ((hdr->attributeMask & BRMI_PAGE_ATTRIBUTE_JOINTS) ? BRMI_CS_JOINTS : 0u)
                      | ((hdr->attributeMask & BRMI_PAGE_ATTRIBUTE_WEIGHTS) ? BRMI_CS_WEIGHTS : 0u);
            if (clusterUv) {      // scenes with textured / alpha-tested materials: UV set 0 of the meshlet and the material's class
                const uint32_t mflags = sc.materials[pm->materialDataIndex].materialFlags;
                const bool layerTextures = openpbr_has_textures(sc.openpbrMaterials + sc.materials[pm->materialDataIndex].openPBRMaterialDataIndex);
                cs.counts |= ((mflags & BRMI_MATERIAL_ALPHA_TEST) ? BRMI_CS_ALPHA : 0u) | (((mflags & BRMI_MATERIAL_ANY_TEXTURE) || layerTextures) ? BRMI_CS_TEXTURED : 0u);
                ClusterUv cu{nullptr, nullptr, nullptr, 0, 0u};
                if (hdr->attributeMask & BRMI_PAGE_ATTRIBUTE_COLOR) { cs.counts |= BRMI_CS_COLOR; cu.color = slab + pageOff + hdr->colorArrayOffset + desc->vertexAttributeOffset * 4u; }
                if (hdr->uvSetCount != 0u) {
                    cu.desc = slab + pageOff + hdr->uvDescriptorOffset + (vc_meshlet(t.packed) * hdr->uvSetCount) * 32u;
                    cu.stream = slab + pageOff + *reinterpret_cast<const uint32_t*>(slab + pageOff + hdr->uvBitstreamDirectoryOffset);
                    cu.directory = (int32_t)hdr->uvBitstreamDirectoryOffset - (int32_t)(hdr->uvDescriptorOffset + (vc_meshlet(t.packed) * hdr->uvSetCount) * 32u);
                    cu.setCount = hdr->uvSetCount;
                }
                clusterUv[dst] = cu;
            }
            cs.jointDelta = (int32_t)(hdr->jointArrayOffset + desc->vertexAttributeOffset * 32u) - (int32_t)(hdr->normalArrayOffset + desc->vertexAttributeOffset * 4u);
            cs.weightDelta = (int32_t)(hdr->weightArrayOffset + desc->vertexAttributeOffset * 32u) - (int32_t)(hdr->normalArrayOffset + desc->vertexAttributeOffset * 4u);
            cs.perObjectIndex = inst.perObjectBufferIndex; cs.instanceIndex = instanceIndex; cs.viewId = vc_view(t.packed);
            cs.materialDataIndex = pm->materialDataIndex; cs.normalMatrixIndex = obj->normalMatrixBufferIndex;
            const unsigned long long v0 = baseV + (inclV - verts), t0 = baseT + (inclT - tris);
            const bool fits = v0 + verts <= resolveCapacity && t0 + tris <= resolveCapacity;
            cs.vertBase = fits ? (uint32_t)v0 : BRMI_ARENA_NONE; cs.triBase32 = fits ? (uint32_t)t0 : BRMI_ARENA_NONE;
            if (!fits && resolveCapacity != 0u) atomicOr(&counters[CNT_RESOLVE_SPILL], 1u);      // selects the G-buffer kernel variant (brmi_gbuffer); (capacity 0 = a frame without tables: flagged once, below -- half a million atomics on one word were 70 us of the 8K frame)
            setup[dst] = cs;
        }
    }
    if (HOLD || dl.countAll) {      // one atomic per wave and launch (the sums are statistics: brmi_algorithmic_bytes)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) drawnVT += (unsigned long long)__shfl_xor((long long)drawnVT, o);
        if ((threadIdx.x & 63u) == 0u && drawnVT != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(&counters[CNT_DRAWN_VT]), drawnVT);
    }
}

static inline uint32_t grid_for(uint64_t items, uint32_t block, uint32_t maxBlocks) {
    uint64_t g = (items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > maxBlocks) g = maxBlocks;
    return (uint32_t)g;
}

// phase 2 starts from the replay buffers: the replayed meshlets become the first bucket records, the replayed nodes the
// level-0 frontier; per-level frontier counters start from zero
__global__ void k_seed_phase2(uint32_t* counters, uint32_t capacity) { seed_phase2(counters, capacity, threadIdx.x); }

int launch_cull(brmi_pass* p, uint32_t phase, hipStream_t s) {
    if (int rc = ensure_frame_constants(p, s)) return rc;
    if (phase != 1 && phase != 2) return fail(p, BRMI_ERR_INVALID, "brmi_cull: phase %u (1 or 2)", phase);
    if (phase == 2 && !p->cfg.enableOcclusionCulling) return fail(p, BRMI_ERR_STATE, "brmi_cull: phase 2 needs a pass created with enableOcclusionCulling");
    if (phase == 2 && !p->hzbValid) return fail(p, BRMI_ERR_STATE, "brmi_cull: phase 2 needs brmi_build_hzb on the phase-1 depth first");
    CullArgs a;
    a.sc = p->scene; a.counters = p->counters();
    a.instanceBitBase = p->wsPtr<uint32_t>(p->ws.instanceBitBase); a.segPrefix = p->wsPtr<uint32_t>(p->ws.segPrefix);
    a.flatNodes = p->wsPtr<FlatNode>(p->ws.flatNodes); a.flatLeaves = p->wsPtr<FlatLeaf>(p->ws.flatLeaves); a.instanceWalk = p->wsPtr<InstanceWalk>(p->ws.instanceWalk);
    a.recordCapacity = p->cfg.maxTraversalRecords; a.visibleCapacity = p->cfg.maxVisibleClusters;
    uint32_t f = p->cfg.phase2ExpansionFactor; f = f < 1 ? 1 : (f > 64 ? 64 : f);
    { uint32_t n = 1; for (uint32_t c = 2; c <= 64; c <<= 1) if (c <= f) n = c; f = n; }
    a.factor = f; a.phase = phase; a.packedFlat = 0u; a.wideFlat = 0u;
    a.feedback = p->ensureFeedback() ? p->phase2FeedbackDev : nullptr;

    // the band test's two planes through the eye only bound a row band under a symmetric perspective projection: an orthographic or
    // off-centre camera keeps the frustum test alone (the rasteriser's row filter still confines the band; nothing is lost but the early cull)
    const bool symmetricPerspective = p->camHost.isOrtho == 0 && p->camHost.projection[2][0] == 0.0f && p->camHost.projection[2][1] == 0.0f &&
                                      p->camHost.projection[3][0] == 0.0f && p->camHost.projection[3][1] == 0.0f;
    a.bandActive = ((p->bandY0 != 0 || p->bandY1 != p->cfg.height) && symmetricPerspective) ? 1u : 0u;
    for (int k = 0; k < 3; k++) { a.bandTop[k] = p->bandPlaneTop[k]; a.bandBottom[k] = p->bandPlaneBottom[k]; }
    a.bandPlanes = reinterpret_cast<const float4*>(p->wsPtr<m4>(p->ws.frameConst) + 3);
    a.stripes = p->stripes;
    const brmi_pass* chain = p->chainOwner(phase);      // frames in flight: phase 1 reads the chain of the pass that rendered the frame before
    a.occlusion = (p->cfg.enableOcclusionCulling && chain->hzbValid && p->camHost.isOrtho == 0) ? 1u : 0u;
    a.replayNodes = p->wsPtr<NodeRecord>(p->ws.replayNodes); a.replayBuckets = p->wsPtr<BucketRecord>(p->ws.replayBuckets);
    a.hzb = chain->hzbDesc();
    if (phase == 1) {
        // Round 6: this frame holds clusters back when the pass can (brmi_set_scene), the previous frame's chain is there to predict from, and the frames before had
        // enough clusters for the two extra launches to pay (the count is a host-mapped word a frame or two old; either way the same image)
        const uint32_t lastVisible = p->phase2FeedbackHost ? reinterpret_cast<volatile uint32_t*>(p->phase2FeedbackHost)[3] : 0u;
        const uint32_t lastPhase2 = p->phase2FeedbackHost ? reinterpret_cast<volatile uint32_t*>(p->phase2FeedbackHost)[0] : 0xFFFFFFFFu;
        // (a still camera's small frame too -- but not a frame of a few hundred clusters: a rank's sky band of 195 clusters pays the three extra launches for nothing; holdFloor)
        p->holdThisFrame = p->holdEnabled && a.occlusion != 0u && (p->holdMinClusters == 0u || (lastVisible != 0xFFFFFFFFu && lastVisible >= p->holdMinClusters) ||
                                                                  (p->holdStillMax != 0u && lastPhase2 < p->holdStillMax && lastVisible != 0xFFFFFFFFu && lastVisible >= p->holdFloor));
    }
    a.frontier0Counter = phase == 1 ? (uint32_t)CNT_FRONTIER0 : (uint32_t)CNT_REPLAY_NODES;
    a.bucketCounter = CNT_BUCKETS;   // phase 2: seeded with the replayed meshlets, the bucket array is the replay buffer itself
    NodeRecord* fa = p->wsPtr<NodeRecord>(p->ws.frontierA); NodeRecord* fb = p->wsPtr<NodeRecord>(p->ws.frontierB);
    BucketRecord* buckets = phase == 1 ? p->wsPtr<BucketRecord>(p->ws.buckets) : a.replayBuckets;
    TempVisible* temp = p->wsPtr<TempVisible>(p->ws.tempVisible);
    uint32_t* bitmask = p->wsPtr<uint32_t>(phase == 1 ? p->ws.bitmask1 : p->ws.bitmask2);
    uint8_t* blockDirty = p->wsPtr<uint8_t>(p->ws.blockDirty) + (phase == 1 ? 0u : p->scanBlocks + 1u);
    uint32_t* wordPrefix = p->wsPtr<uint32_t>(p->ws.wordPrefix); uint32_t* blockSums = p->wsPtr<uint32_t>(p->ws.blockSums);

    // brmi_set_streaming: the same launches with the residency rule compiled in (the trailing argument's type selects the variant)
    const StreamArgs st = stream_args_of(p);
#define BRMI_LAUNCH_CULL(KERNEL, KERNEL_STREAMING, GRID, BLOCK, ...) do { if (p->streaming.on) hipLaunchKernelGGL(KERNEL_STREAMING, GRID, BLOCK, 0, s, __VA_ARGS__, st); else hipLaunchKernelGGL(KERNEL, GRID, BLOCK, 0, s, __VA_ARGS__); } while (0)
    const uint32_t maxBlocks = 1024;
    bool lightGridRides = false;      // this call's launches carry the light clustering (brmi_execute)
    bool flatLevels = false;          // phase 1 ran the level-synchronous flat traversal: nothing is left for the walk or the level kernels
    // one launch of k_cull_hierarchy for the meshes that fit its LDS frontier, the level kernels for the rest (or for everything: tests)
    const bool hierarchy = p->minLevelWidth <= HIER_CAP_MAX && !p->forceLevelKernels;
    const bool levelKernels = p->maxLevelWidth > p->spillWidth || p->forceLevelKernels;
    const uint32_t* meshWidth = p->wsPtr<uint32_t>(p->ws.meshLevelWidth);
    // meshes of both kinds: the one-launch walk also starts the wide ones and hands their frontiers to the level kernels (spill mode)
    const bool spillMode = hierarchy && levelKernels;
    a.meshLevelWidth = meshWidth; a.levelKernelsWidthLo = 0u;
    if (spillMode) a.frontier0Counter = CNT_FRONTIER0;
    const uint32_t widthAll = spillMode ? 0xFFFFFFFFu : 0u, spillAbove = spillMode ? p->spillWidth : 0xFFFFFFFFu;
    if (phase == 1) {
        if (!p->frameStateCleared) BRMI_HIP(p, hipMemsetAsync(p->counters(), 0, p->ws.frameClearBytes, s));      // counters + both survivor bitmasks
        p->frameStateCleared = false;
        // (CLodStreamingBeginFramePass: the frame's touched bits and best requests start from zero)
        if (p->streaming.on) BRMI_HIP(p, hipMemsetAsync(p->streaming.b.scratch, 0, stream_scratch_layout(p->streaming.groupCount).frameBytes, s));
        // (the first ceil(draws / 8) waves of the walk take eight draws each: hierarchies of <= 8 nodes, the flat tables of brmi_set_scene)
        a.packedFlat = (hierarchy && !p->hostFlatNodes.empty() && p->packedFlat) ? 1u : 0u;
        // (not beside another frame's shading half: a 1024-thread workgroup with 40 KB of LDS waits long for a CU that can take it, and the
        // dense frame in flight went 0.795 -> 0.91 ms; alone the same frame's cull stage goes 0.180 -> 0.142 ms)
        a.wideFlat = (hierarchy && p->anyWideFlat && !p->splitFrame) ? 1u : 0u;
        // Scenes of very many draws (Zorah-class): the level-synchronous flat traversal, a lane per (instance, node) task, one launch per level of the
        // deepest hierarchy (k_cull_flat_level).  Its launches carry no riders: the visibility clear moves onto k_cull_clusters (ClearRide) and the
        // light clustering is launched by the frame where it finds none done.
        // (also, from a quarter of that count on, in a SPLIT frame of a scene whose hierarchies need the 24 KB-frontier variant of the walk: its single-wave workgroups of 150 registers
        // and 24 KB of LDS find few slots beside another frame's shading waves -- San-Miguel-class, 7,577 draws: 0.848 -> 0.823 ms in flight although the stage alone is 0.107 -> 0.119;
        // the dense and Bistro-class frames, with fewer draws, lose either way)
        const uint32_t draws = p->scene.activeDrawCount, minDraws = std::max(1u, p->flatLevelsMinDraws);
        flatLevels = hierarchy && p->allMeshesFlat && !p->forceLevelKernels && (draws >= minDraws || (p->splitFrame && p->maxLevelWidth > 256u && draws >= std::max(1u, minDraws / 4u)));
        if (flatLevels) {
            if (p->clearVisibilityWithTraversal && (p->bandPixelCount & 1ull) == 0ull) { p->clearVisibilityWithTraversal = false; p->clearVisibilityWithClusterCull = true; }
            else if (p->clearVisibilityWithTraversal) flatLevels = false;      // (an odd pixel count: the riding clear of the walk handles it)
        }
        if (flatLevels) {
            BRMI_LAUNCH_CULL((k_cull_flat_level<true>), (k_cull_flat_level_streaming<true>), dim3(grid_for(p->scene.activeDrawCount, 256, 8192)), dim3(256), a, 0u, (const NodeRecord*)nullptr, fb, buckets);
            // (frontier sizes live on the device; every level strides a fixed grid and a workgroup that finds none of its tasks leaves after one load)
            for (uint32_t level = 1; level < p->flatMaxDepth; level++)
                BRMI_LAUNCH_CULL((k_cull_flat_level<false>), (k_cull_flat_level_streaming<false>), dim3(2048), dim3(256), a, level, (const NodeRecord*)((level & 1u) ? fb : fa), (level & 1u) ? fa : fb, buckets);
            BRMI_LAUNCH_CHECK(p, "k_cull_flat_level");
        }
        const dim3 hgrid(std::min(std::max(1u, p->scene.activeDrawCount), 16384u) + (a.packedFlat ? (p->scene.activeDrawCount + 7u) / 8u : 0u));
        if (hierarchy && !flatLevels) {
            // ONE launch: the 6 KB-frontier variant when every mesh is narrow (<= 256 nodes per level), else the 24 KB variant for all meshes up
            // to 1024 (two launches, one per class, ran one after the other: San-Miguel-class cull 178 -> 140 us with one)
            const bool wide = p->maxLevelWidth > 256u;
            const uint32_t widthHi = spillMode ? widthAll : (wide ? HIER_CAP_MAX : 256u);
            if (p->clearVisibilityWithTraversal) {
                SideJobs sj{reinterpret_cast<ulonglong2*>(static_cast<unsigned long long*>(p->res[BRMI_RES_VISIBILITY]) + p->bandFirstPixel), p->bandPixelCount >> 1, hgrid.x, p->clearRiderBlocks, cluster_args_of(p)};
                const dim3 grid(hgrid.x + sj.clearBlocks + p->numLightClusters);
                if (wide) BRMI_LAUNCH_CULL((k_cull_hierarchy<false, 1024, BRMI_HIER_STAGE_WIDE, true>), (k_cull_hierarchy_streaming<false, 1024, BRMI_HIER_STAGE_WIDE, true>), grid, dim3(64), a, buckets, meshWidth, 0u, widthHi, spillAbove, fa, sj);
                else BRMI_LAUNCH_CULL((k_cull_hierarchy<false, 256, 128, true>), (k_cull_hierarchy_streaming<false, 256, 128, true>), grid, dim3(64), a, buckets, meshWidth, 0u, widthHi, spillAbove, fa, sj);
                p->clearVisibilityWithTraversal = false; lightGridRides = true;
            } else if (wide) BRMI_LAUNCH_CULL((k_cull_hierarchy<false, 1024, BRMI_HIER_STAGE_WIDE, false>), (k_cull_hierarchy_streaming<false, 1024, BRMI_HIER_STAGE_WIDE, false>), hgrid, dim3(64), a, buckets, meshWidth, 0u, widthHi, spillAbove, fa, NoSide{});
            else BRMI_LAUNCH_CULL((k_cull_hierarchy<false, 256, 128, false>), (k_cull_hierarchy_streaming<false, 256, 128, false>), hgrid, dim3(64), a, buckets, meshWidth, 0u, widthHi, spillAbove, fa, NoSide{});
        }
        if (a.wideFlat && !flatLevels) BRMI_LAUNCH_CULL(k_cull_flat_wide, k_cull_flat_wide_streaming, dim3(std::min(std::max(1u, p->scene.activeDrawCount), 4096u)), dim3(1024), a, buckets);
        if (levelKernels && !spillMode && !flatLevels) hipLaunchKernelGGL(k_cull_instances, dim3(grid_for(p->scene.activeDrawCount, 256, maxBlocks)), dim3(256), 0, s, a, fa);
        BRMI_LAUNCH_CHECK(p, "k_cull_instances");
    } else {
        // brmi_execute seeds in the tail of the depth-chain build that precedes this call (one launch less)
        if (!p->phase2Seeded) hipLaunchKernelGGL(k_seed_phase2, dim3(1), dim3(128), 0, s, p->counters(), a.recordCapacity);
        p->phase2Seeded = false;
        const NoSide none{};
        if (hierarchy && p->maxLevelWidth <= 256u) BRMI_LAUNCH_CULL((k_cull_hierarchy<true, 256, 128, false>), (k_cull_hierarchy_streaming<true, 256, 128, false>), dim3(2048), dim3(64), a, buckets, meshWidth, 0u, 256u, spillAbove, fa, none);
        else if (hierarchy) BRMI_LAUNCH_CULL((k_cull_hierarchy<true, 1024, BRMI_HIER_STAGE_WIDE, false>), (k_cull_hierarchy_streaming<true, 1024, BRMI_HIER_STAGE_WIDE, false>), dim3(2048), dim3(64), a, buckets, meshWidth, 0u, spillMode ? widthAll : HIER_CAP_MAX, spillAbove, fa, none);
    }
    // frontier sizes are only known on the device: size the grids for the worst case that can matter
    const uint32_t travGrid = grid_for(std::min<uint64_t>(p->cfg.maxTraversalRecords, (uint64_t)p->scene.lodNodeCount * 4 + 4096), 256, maxBlocks);
    const uint32_t levelLaunches = spillMode ? std::min(p->maxLevels, std::max(1u, p->spillLevels)) : p->maxLevels;
    // (phase 1 of a scene whose every hierarchy is evaluated flat leaves nothing for the level kernels)
    const bool flatCoversPhase1 = phase == 1 && hierarchy && spillMode && p->allMeshesFlat && a.wideFlat != 0u && !p->forceLevelKernels;
    for (uint32_t level = 0; level < levelLaunches && levelKernels && !flatCoversPhase1 && !flatLevels; level++) {
        // without the walk in front (forced level kernels) phase 2 reads level 0 from the replay buffer; then ping-pong like phase 1 (level 0 writes fb)
        const NodeRecord* in = level == 0 ? ((phase == 1 || spillMode) ? fa : a.replayNodes) : ((level & 1u) ? fb : fa);
        BRMI_LAUNCH_CULL(k_traverse, k_traverse_streaming, dim3(travGrid), dim3(256), a, level, in, (level & 1u) ? fa : fb, buckets);
        BRMI_LAUNCH_CHECK(p, "k_traverse");
    }
    // grid-stride kernels that usually find little to do: a few hundred workgroups retire in ~3 us, a thousand in ~6
    // Frames of hundreds of thousands of records (Zorah-class: 180 k bucket records, 490 k survivors) need more than that: a lane's chain of dependent loads
    // (record -> page header -> descriptor -> instance -> object -> depth chain) three or four times over was most of both kernels.  The counts of the frames
    // before (host-mapped words the kernels write; read without waiting, any value is safe: the kernels stride their grids) size the launches.
    uint32_t smallGrid = phase == 1 ? 512u : 128u, scatterGrid = smallGrid;
    if (p->phase2FeedbackHost) {
        const uint32_t lastBuckets = reinterpret_cast<volatile uint32_t*>(p->phase2FeedbackHost)[phase == 1 ? 2 : 4];
        const uint32_t lastVisible = reinterpret_cast<volatile uint32_t*>(p->phase2FeedbackHost)[phase == 1 ? 3 : 0];      // (0xFFFFFFFF = unknown is clamped below)
        smallGrid = std::max(smallGrid, grid_for((uint64_t)std::min<uint32_t>(lastBuckets, p->cfg.maxTraversalRecords) * f, 256, 8192));
        scatterGrid = std::max(scatterGrid, grid_for(std::min<uint32_t>(lastVisible, p->cfg.maxVisibleClusters), 256, 8192));
    }
    if (lightGridRides) {
        BRMI_LAUNCH_CULL((k_cull_clusters<1>), (k_cull_clusters_streaming<1>), dim3(smallGrid + (p->numLightClusters + 3u) / 4u), dim3(256), a, (const BucketRecord*)buckets, temp, bitmask, blockDirty, LcRide{smallGrid, cluster_args_of(p)});
        p->lightGridDone = true;
    } else if (phase == 1 && p->clearVisibilityWithClusterCull) {
        const uint32_t clearBlocks = 2048;
        BRMI_LAUNCH_CULL((k_cull_clusters<2>), (k_cull_clusters_streaming<2>), dim3(smallGrid + clearBlocks), dim3(256), a, (const BucketRecord*)buckets, temp, bitmask, blockDirty,
                           ClearRide{smallGrid, reinterpret_cast<ulonglong2*>(static_cast<unsigned long long*>(p->res[BRMI_RES_VISIBILITY]) + p->bandFirstPixel), p->bandPixelCount >> 1, clearBlocks});
        p->clearVisibilityWithClusterCull = false;
    } else BRMI_LAUNCH_CULL((k_cull_clusters<0>), (k_cull_clusters_streaming<0>), dim3(smallGrid), dim3(256), a, (const BucketRecord*)buckets, temp, bitmask, blockDirty, NoSide{});
    BRMI_LAUNCH_CHECK(p, "k_cull_clusters");
    // phase 2 appends behind the phase-1 clusters: its capacity is what phase 1 left
    const uint32_t outIndex = phase == 1 ? CNT_VISIBLE : CNT_VISIBLE2, usedIndex = phase == 1 ? 0xFFFFFFFFu : (uint32_t)CNT_VISIBLE;
    // every workgroup of the scatter scanning the bitmask itself pays off while the bitmask is small (BASELINE-class scenes: ~1-4 k words);
    // from 8 k words on the three scan launches are faster (dense frame, 25 k words: 27 us against 55 us per phase)
    // phase 2: the ranking kernel also tells the host how many clusters it placed (launch_raster's hint for the frames that follow)
    if (phase == 2 && p->phase2DirectMax != 0u) (void)p->ensureFeedback();
    uint32_t* feedback = phase == 2 ? p->phase2FeedbackDev : (p->phase2FeedbackDev ? p->phase2FeedbackDev + 3 : nullptr);      // (phase 1: word 3, the sizes of the next frames' launches)
    const bool localRank = p->totalWords <= LOCAL_RANK_WORDS && !p->forceLevelKernels;
    if (localRank) {
        // ranked inside the scatter kernel
    } else {
        if (p->scanBlocks <= SCAN_CHAIN_BLOCKS) {
            if (++p->scanEpoch == 0u) p->scanEpoch = 1u;
            hipLaunchKernelGGL(k_scan_chained, dim3(p->scanBlocks), dim3(256), 0, s, bitmask, p->totalWords, p->wsPtr<unsigned long long>(p->ws.scanAgg), p->scanEpoch, wordPrefix,
                               p->counters(), outIndex, p->cfg.maxVisibleClusters, usedIndex, feedback);
        } else {
            hipLaunchKernelGGL(k_scan_reduce, dim3(p->scanBlocks), dim3(256), 0, s, bitmask, p->totalWords, blockSums, blockDirty);
            hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, blockSums, p->scanBlocks, p->counters(), outIndex, p->cfg.maxVisibleClusters, usedIndex, feedback);
            hipLaunchKernelGGL(k_scan_words, dim3(p->scanBlocks), dim3(256), 0, s, bitmask, p->totalWords, blockSums, wordPrefix, blockDirty);
        }
    }
    // (a frame whose G-buffer pass works without the per-cluster tables reserves nothing in the resolve arena: every cluster is marked "no tables")
    if (phase == 1) p->inlineResolve = resolve_inline_frame(p);
    const uint32_t arenaCapacity = p->inlineResolve ? 0u : p->resolveCapacity;
    auto scatter = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(scatterGrid), dim3(256), 0, s, temp, p->counters(), (uint32_t)(phase == 1 ? CNT_TEMP_VISIBLE : CNT_TEMP_VISIBLE2), bitmask, wordPrefix,
                           static_cast<uint4*>(p->res[BRMI_RES_VISIBLE_CLUSTERS]), phase == 1 ? 0xFFFFFFFFu : (uint32_t)CNT_VISIBLE, p->cfg.maxVisibleClusters, p->cfg.maxVisibleClusters, p->scene, p->wsPtr<ClusterSetup>(p->ws.clusterSetup), arenaCapacity,
                           (p->sceneHasTextures || p->sceneHasAlphaTest || p->sceneHasVertexColors) ? p->wsPtr<ClusterUv>(p->ws.clusterUv) : nullptr, LocalRank{p->totalWords, outIndex, usedIndex, feedback},
                           (phase == 1 && p->holdThisFrame) ? DrawLists{p->wsPtr<uint32_t>(p->ws.drawList), p->wsPtr<HeldRecord>(p->ws.heldRecords), 0u, p->wsPtr<MeshletBox>(p->ws.meshletBoxes), p->wsPtr<uint32_t>(p->ws.pageBoxBase),
                                                                      p->wsPtr<float>(p->ws.objConst), p->holdMaxTexels, BoxViewport{(float)p->cfg.width, (float)p->cfg.height, 0.0f, 0.0f, 0, (int)p->bandY0, (int)p->cfg.width - 1, (int)p->bandY1 - 1}, a.hzb}
                                                          : DrawLists{nullptr, nullptr, p->holdThisFrame ? 1u : 0u, nullptr, nullptr, nullptr, 0u, BoxViewport{}, HzbDesc{}});
    };
    const bool holdLists = phase == 1 && p->holdThisFrame;
    if (localRank) { if (holdLists) scatter(k_scatter_visible<true, true>); else scatter(k_scatter_visible<true, false>); }
    else { if (holdLists) scatter(k_scatter_visible<false, true>); else scatter(k_scatter_visible<false, false>); }
    BRMI_LAUNCH_CHECK(p, "compaction");
    return BRMI_OK;
#undef BRMI_LAUNCH_CULL
}


// Round 6: the object-space box of every meshlet of every resident page (brmi_setup; MeshletBox in brmi_internal.h).  One workgroup per page, a wave per meshlet.
__global__ void __launch_bounds__(256) k_meshlet_boxes(const uint8_t* const* slabs, const PageRef* pages, MeshletBox* boxes) {
    const PageRef pr = pages[blockIdx.x];
    const uint8_t* page = slabs[pr.slab] + pr.byteOffset;
    const brmi_page_header* hdr = reinterpret_cast<const brmi_page_header*>(page);
    const uint32_t lane = threadIdx.x & 63u;
    const bool float3 = (hdr->compressedPositionQuantExp & 0xFFu) == BRMI_POSITION_FORMAT_FLOAT3;
    for (uint32_t m = threadIdx.x >> 6; m < pr.meshletCount; m += 4u) {
        const brmi_meshlet_descriptor* desc = reinterpret_cast<const brmi_meshlet_descriptor*>(page + hdr->descriptorOffset + m * 64u);
        const uint32_t verts = min((desc->bitsAndVertexCount >> 24) & 0xFFu, BRMI_MESHLET_MAX_VERTS);
        f3 lo{3.0e38f, 3.0e38f, 3.0e38f}, hi{-3.0e38f, -3.0e38f, -3.0e38f};
        bool finite = true;
        if (float3) for (uint32_t v = lane; v < verts; v += 64u) {
            const float* pp = reinterpret_cast<const float*>(page + hdr->positionBitstreamOffset + desc->positionBitOffset + v * 12u);
            const f3 q{pp[0], pp[1], pp[2]};
            finite = finite && fabsf(q.x) < 1.0e30f && fabsf(q.y) < 1.0e30f && fabsf(q.z) < 1.0e30f;      // (NaN fails the comparison)
            lo = min3v(lo, q); hi = max3v(hi, q);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo.x = min2(lo.x, __shfl_xor(lo.x, o)); lo.y = min2(lo.y, __shfl_xor(lo.y, o)); lo.z = min2(lo.z, __shfl_xor(lo.z, o));
            hi.x = max2(hi.x, __shfl_xor(hi.x, o)); hi.y = max2(hi.y, __shfl_xor(hi.y, o)); hi.z = max2(hi.z, __shfl_xor(hi.z, o));
        }
        finite = __all(finite);
        if (lane == 0u) boxes[pr.boxBase + m] = MeshletBox{{lo.x, lo.y, lo.z}, (float3 && verts != 0u && finite) ? 1u : 0u, {hi.x, hi.y, hi.z}, 0u};
    }
}

int launch_meshlet_boxes(brmi_pass* p, hipStream_t s) {
    if (p->hostPageRefs.empty()) return BRMI_OK;
    hipLaunchKernelGGL(k_meshlet_boxes, dim3((uint32_t)p->hostPageRefs.size()), dim3(256), 0, s, p->scene.slabs, p->wsPtr<PageRef>(p->ws.pageRefs), p->wsPtr<MeshletBox>(p->ws.meshletBoxes));
    BRMI_LAUNCH_CHECK(p, "k_meshlet_boxes");
    return BRMI_OK;
}

// ---- brmi_streaming_feedback: the counterpart of CLodStreamingFeedbackSortPass ------------------------------------------------------------
// Input: the frame's touched bits and best request per group (stream_touch).  Output (include/brmi.h): the touched groups in ascending order, and one
// record per requested group ordered by descending priority, then ascending group.  The reference sorts up to 65,536 appended records, most of them
// duplicates, with a device radix sort; a frame here has at most one request per group, already in group order after the compaction, so two stable
// 8-bit counting passes over the inverted priority order them.  One 1024-thread workgroup: a frame asks for hundreds to a few thousand groups, and the
// passes over the group table (a bit and a word per group) are a few rounds of coalesced loads.
BRMI_DEV uint32_t block_exclusive_scan_1024(uint32_t v, uint32_t* waveTotals /* [17] */, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o); if (lane >= (uint32_t)o) incl += t; }
    __syncthreads();                                    // the previous round's totals have been read
    if (lane == 63u) waveTotals[wave] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (uint32_t w = 0; w < 16u; w++) { if (w < wave) base += waveTotals[w]; all += waveTotals[w]; }
    total = all;
    return base + incl - v;
}

__global__ void __launch_bounds__(1024) k_stream_feedback(StreamArgs st, uint32_t* listA, uint32_t* listB, brmi_streaming_request* loadRequests, uint32_t requestCapacity,
                                                          uint32_t* touchedGroups, uint32_t touchedCapacity, uint32_t* counts, const brmi_per_mesh_instance* instances, uint32_t instanceCount,
                                                          const brmi_per_frame* perFrame) {
    __shared__ uint32_t waveTotals[17], digitBase[256], digitHist[256];
    __shared__ uint16_t waveDigit[16][256];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t groups = st.groupCount, words = (groups + 31u) >> 5;
    // touched groups, ascending
    uint32_t carry = 0;
    for (uint32_t base = 0; base < words; base += 1024u) {
        const uint32_t w = base + t;
        uint32_t bits = w < words ? st.touchedBits[w] : 0u;
        if (w == words - 1u && (groups & 31u)) bits &= (1u << (groups & 31u)) - 1u;
        uint32_t total;
        uint32_t slot = carry + block_exclusive_scan_1024((uint32_t)__popc(bits), waveTotals, total);
        for (; bits != 0u; bits &= bits - 1u, slot++) if (slot < touchedCapacity) touchedGroups[slot] = w * 32u + (uint32_t)__ffs((int)bits) - 1u;
        carry += total;
    }
    if (t == 0) counts[1] = carry;
    // requested groups, ascending
    uint32_t requests = 0;
    for (uint32_t base = 0; base < groups; base += 1024u) {
        const uint32_t g = base + t;
        const bool has = g < groups && st.requestKeys[g] != 0ull;
        uint32_t total;
        const uint32_t slot = requests + block_exclusive_scan_1024(has ? 1u : 0u, waveTotals, total);
        if (has) listA[slot] = g;
        requests += total;
    }
    if (t == 0) counts[0] = requests;
    // two stable counting passes: low, then high byte of 0xFFFF - priority16
    uint32_t* src = listA; uint32_t* dst = listB;
    for (uint32_t shift = 0; shift < 16u; shift += 8u) {
        __syncthreads();                                // the list is complete (global stores of this workgroup, read back by it)
        __threadfence_block();
        if (t < 256u) digitHist[t] = 0u;
        __syncthreads();
        for (uint32_t i = t; i < requests; i += 1024u) atomicAdd(&digitHist[((0xFFFFu - ((uint32_t)(st.requestKeys[src[i]] >> 32) & 0xFFFFu)) >> shift) & 0xFFu], 1u);
        __syncthreads();
        if (wave == 0u) {                               // exclusive scan of the 256 digit counts: four per lane
            const uint32_t c0 = digitHist[lane * 4u], c1 = digitHist[lane * 4u + 1u], c2 = digitHist[lane * 4u + 2u], c3 = digitHist[lane * 4u + 3u];
            uint32_t incl = c0 + c1 + c2 + c3;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)incl, o); if (lane >= (uint32_t)o) incl += v; }
            const uint32_t excl = incl - (c0 + c1 + c2 + c3);
            digitBase[lane * 4u] = excl; digitBase[lane * 4u + 1u] = excl + c0; digitBase[lane * 4u + 2u] = excl + c0 + c1; digitBase[lane * 4u + 3u] = excl + c0 + c1 + c2;
        }
        for (uint32_t base = 0; base < requests; base += 1024u) {
            __syncthreads();                            // digitBase is current, the previous round's table has been read
            for (uint32_t k = t; k < 16u * 256u; k += 1024u) (&waveDigit[0][0])[k] = 0;
            __syncthreads();
            const uint32_t i = base + t;
            const bool valid = i < requests;
            const uint32_t g = valid ? src[i] : 0u;
            const uint32_t d = valid ? ((0xFFFFu - ((uint32_t)(st.requestKeys[g] >> 32) & 0xFFFFu)) >> shift) & 0xFFu : 0u;
            uint64_t same = __ballot(valid);            // lanes of this wave with the same digit
#pragma unroll
            for (uint32_t b = 0; b < 8u; b++) { const uint64_t m = __ballot(valid && ((d >> b) & 1u)); same &= ((d >> b) & 1u) ? m : ~m; }
            const uint32_t rankInWave = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
            if (valid && rankInWave == 0u) waveDigit[wave][d] = (uint16_t)__popcll(same);
            __syncthreads();
            if (valid) {
                uint32_t before = 0;
                for (uint32_t w = 0; w < wave; w++) before += waveDigit[w][d];
                dst[digitBase[d] + before + rankInWave] = g;
            }
            __syncthreads();
            if (t < 256u) { uint32_t all = 0; for (uint32_t w = 0; w < 16u; w++) all += waveDigit[w][t]; digitBase[t] += all; }
        }
        uint32_t* x = src; src = dst; dst = x;
    }
    __syncthreads();
    __threadfence_block();
    const uint32_t view = perFrame->mainCameraIndex;
    for (uint32_t i = t; i < min(requests, requestCapacity); i += 1024u) {
        const uint32_t g = src[i];
        const unsigned long long key = st.requestKeys[g];
        const uint32_t inst = ~(uint32_t)key, priority16 = (uint32_t)(key >> 32) & 0xFFFFu;
        brmi_streaming_request r;
        r.groupGlobalIndex = g; r.meshInstanceIndex = inst; r.meshBufferIndex = inst < instanceCount ? instances[inst].perMeshBufferIndex : 0u;
        r.viewId = (priority16 << 16) | (view & 0xFFFFu);
        loadRequests[i] = r;
    }
}

int launch_streaming_feedback(brmi_pass* p, hipStream_t s) {
    const StreamScratchLayout l = stream_scratch_layout(p->streaming.groupCount);
    uint8_t* scratch = static_cast<uint8_t*>(p->streaming.b.scratch);
    hipLaunchKernelGGL(k_stream_feedback, dim3(1), dim3(1024), 0, s, stream_args_of(p), reinterpret_cast<uint32_t*>(scratch + l.listA), reinterpret_cast<uint32_t*>(scratch + l.listB),
                       p->streaming.b.loadRequests, p->streaming.b.requestCapacity, p->streaming.b.touchedGroups, p->streaming.b.touchedCapacity, p->streaming.b.counts,
                       p->scene.perMeshInstance, p->scene.perMeshInstanceCount, p->scene.perFrame);
    BRMI_LAUNCH_CHECK(p, "k_stream_feedback");
    return BRMI_OK;
}

}  // namespace brmi
