// brmi_scene_tables.h -- everything brmi_set_scene derives from a scene, as host-only code: index arithmetic on host copies of the scene's
// arrays.  No HIP here (this header compiles with a plain C++17 compiler and runs under the host sanitizers, tests/scene_tables_main.cpp):
// brmi_set_scene copies each device array to a HostScene once and calls analyse_scene; the result is brmi_pass::tables.
#ifndef BRMI_SCENE_TABLES_H
#define BRMI_SCENE_TABLES_H

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "brmi.h"

namespace brmi {

// The two indices of the device-visible counters block (brmi_internal.h, CounterIndex) that bound the depth of a flat hierarchy
constexpr uint32_t CNT_FRONTIER0 = 32;        // frontier sizes per BFS level: [CNT_FRONTIER0 + level]
constexpr uint32_t CNT_STRIPES = 128;         // 64 stripes x 32 words: per-stripe {instances tested, instances visible, nodes visited}

// internal records (ours; the reference's 12 B / 24 B records plus the rank bookkeeping)
// A mesh whose whole BVH has at most 8192 nodes (build_flat_tables walks it) is evaluated flat by the traversal kernels: one lane per node (a wave for
// up to 256 nodes, eight draws to a wave up to 8, a 1024-thread workgroup beyond 256), the
// records below instead of the node -> group / segment chain (static topology: node, group and segment contents as brmi_set_scene read them;
// what the host may rewrite between frames -- instances, objects, the page map -- is still read from its buffers).
struct FlatNode {                                                                     // 64 B, breadth-first (a parent's position is below its children's)
    float cull[4], lod[4]; float maxQuadricError;
    uint32_t nodeId;            // relative to the mesh's lodNodesBase (replay records name nodes by it)
    uint32_t info;              // internal | has a refined group << 1 | segment holds meshlets << 2 | parent position << 8 (breadth-first: below the node's own)
    uint32_t ownerGroup;        // leaf: mesh-local group
    uint32_t segFirstCount;     // leaf: firstMeshletInPage | meshletCount << 16
    uint32_t pageMapIndex;      // leaf: absolute index of the segment's page-map entry
    uint32_t firstBitRel;       // leaf: the segment's first bit relative to the instance's
    uint32_t children;          // internal: position of the first child | child count << 16 (breadth-first: a node's children sit side by side)
};
struct FlatLeaf { float group[4], child[4]; float childParentError; uint32_t ownerGlobal, childGlobal /* indices into lodGroups: what the residency rule looks up (brmi_set_streaming) */, pad; };      // 48 B: the leaf's group sphere, its refined group's sphere and error
struct InstanceWalk { uint32_t flatBase, flatCount /* 0: the level walk */, bitBase, skinned; };                                    // 16 B per mesh instance
static_assert(sizeof(FlatNode) == 64 && sizeof(FlatLeaf) == 48 && sizeof(InstanceWalk) == 16, "flat traversal records");
struct PageRef { uint32_t slab, byteOffset, boxBase, meshletCount; };                 // one resident page (build_page_table walks the page map)
static_assert(sizeof(PageRef) == 16, "draw-list records");

// Host copies of the scene arrays the analysis reads (brmi_scene_buffers: same names, same element types).
struct HostScene {
    std::vector<brmi_clod_mesh_metadata> meshMetadata; std::vector<brmi_lod_node> lodNodes; std::vector<brmi_lod_segment> lodSegments; std::vector<brmi_lod_group> lodGroups;
    std::vector<brmi_group_page_map_entry> groupPageMap; std::vector<brmi_material_info> materials; std::vector<brmi_openpbr_material_info> openpbrMaterials;
    std::vector<brmi_per_mesh> perMesh; std::vector<brmi_per_mesh_instance> perMeshInstance; std::vector<brmi_mesh_instance_clod_offsets> clodOffsets;      // clodOffsets: one per mesh instance, as long as perMeshInstance
    std::vector<uint32_t> activeDraws;
    std::vector<const uint8_t*> slabs;      // the slab pointer table, entry 0 included; null = not resident.  Only build_page_table's reader follows a pointer
    uint32_t perObjectCount = 0, skinningMatrixCount = 0;
    bool textureTables = false;             // textures, samplers and the sRGB decode table are all there (non-null, non-zero counts)
};

struct SceneTables {
    // classify_materials: which kernel variants and workspace tables the scene can need (materials edited on the device later: call brmi_set_scene again)
    bool hasCoat = true, hasFuzz = true;   // some OpenPBR material has a coat / fuzz layer
    bool hasAlphaTest = false, hasTextures = false, hasParallax = false;   // some material is alpha tested / samples a texture / carries a parallax height map
    bool hasVertexColors = false;          // some mesh's pages carry vertex colours (perMesh.vertexFlags bit 0)
    uint32_t uvSets = 1;                   // UV sets the texture slots of the scene's materials name
    // build_rank_tables: the static rank tables of the deterministic visible-cluster compaction and the shape of the hierarchies
    std::vector<uint32_t> segPrefix, instanceBitBase;      // per segment: meshlets of the mesh's segments before it; per mesh instance: its first bit of the survivor bitmask
    uint64_t totalBits = 0; uint32_t maxDepth = 1;         // (instance, meshlet) pairs of the scene; levels of the deepest BVH
    static constexpr uint32_t spillWidth = 1024;      // meshes with a BVH level wider than this go to the level kernels below their top (<= the widest LDS frontier)
    uint32_t spillLevels = 0;        // level-kernel launches the widest meshes still need below the point where the LDS walk hands them over
    uint32_t minLevelWidth = 0;      // narrowest such width over the meshes
    std::vector<uint32_t> meshLevelWidth;   // per mesh metadata entry
    uint32_t maxLevelWidth = 0;      // widest BVH level of any mesh (decides between the per-instance and the per-level traversal)
    // build_flat_tables
    std::vector<FlatNode> flatNodes; std::vector<FlatLeaf> flatLeaves; std::vector<InstanceWalk> instanceWalk;
    bool anyWideFlat = false, allMeshesFlat = false;      // some mesh has 257 .. 8192 nodes / every mesh has flat tables
    uint32_t flatMaxDepth = 1;       // levels of the deepest flat hierarchy (launches of the level-synchronous flat traversal, brmi_cull.hip: k_cull_flat_level)
    // build_page_table.  Round 6, the draw list: per-meshlet boxes of the scene's resident pages (brmi_raster.hip)
    std::vector<PageRef> pageRefs; std::vector<uint32_t> pageBoxBase; uint32_t totalBoxes = 0;
};

// the meshlet count of a resident page: the first word of its header, `byteOffset` bytes into slab `slab`.  Returns a brmi_status.
using PageHeaderReader = std::function<int(uint32_t slab, uint32_t byteOffset, uint32_t* meshlets)>;

// the one formatter of error texts (brmi_api.hip: fail): `msg` becomes the text, `code` comes back
inline int vrefuse(std::string& msg, int code, const char* fmt, va_list ap) { char buf[512]; vsnprintf(buf, sizeof(buf), fmt, ap); msg = buf; return code; }
inline int refuse(std::string& msg, int code, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vrefuse(msg, code, fmt, ap); va_end(ap); return code; }

inline int classify_materials(const HostScene& hs, SceneTables& t, std::string& msg) {
    t.hasCoat = t.hasFuzz = false;
    bool layerTextures = false;
    // UV sets the G-buffer pass must decode: 1 + the highest set an enabled texture slot names (AppendClodMaterialUvSample: an index >= 8 reads set 0)
    uint32_t uvSets = 1;
    auto names_set = [&](uint32_t setIndex) { if (setIndex < 8u && setIndex + 1u > uvSets) uvSets = setIndex + 1u; };
    for (const brmi_openpbr_material_info& m : hs.openpbrMaterials) {
        if (m.coatWeight > 0.0f) t.hasCoat = true;
        if (m.fuzzWeight > 0.0f) t.hasFuzz = true;
        // HasOpenPBRTexture (utilities.hlsli:643-646): a coat / fuzz slot with a valid texture AND sampler index is sampled
        for (int k = 0; k < 6; k++)
            if (m.textureBindings[2 * k] != 0xFFFFFFFFu && m.textureBindings[2 * k + 1] != 0xFFFFFFFFu) {
                layerTextures = true;
                names_set(m.textureBindings[26 + k]);
            }
    }
    // texture slots: the alpha-test variants of the rasteriser and the texture-sampling variant of the G-buffer pass are only
    // launched for scenes that need them
    t.hasAlphaTest = false; t.hasTextures = layerTextures; t.hasParallax = false;
    for (const brmi_material_info& m : hs.materials) {
        if (m.materialFlags & BRMI_MATERIAL_PARALLAX) names_set(m.heightUvSetIndex);
        if (m.materialFlags & BRMI_MATERIAL_ALPHA_TEST) t.hasAlphaTest = true;
        if (m.materialFlags & BRMI_MATERIAL_PARALLAX) t.hasParallax = true;
        if (m.materialFlags & BRMI_MATERIAL_ANY_TEXTURE) {
            t.hasTextures = true;
            const uint32_t f = m.materialFlags;
            if (f & BRMI_MATERIAL_BASE_COLOR_TEXTURE) names_set(m.baseColorUvSetIndex);
            if (f & BRMI_MATERIAL_NORMAL_MAP) names_set(m.normalUvSetIndex);
            if (f & BRMI_MATERIAL_METALLIC_TEXTURE) names_set(m.metallicUvSetIndex);
            if (f & BRMI_MATERIAL_ROUGHNESS_TEXTURE) names_set(m.roughnessUvSetIndex);
            if (f & BRMI_MATERIAL_EMISSIVE_TEXTURE) names_set(m.emissiveUvSetIndex);
            if (f & BRMI_MATERIAL_AO_TEXTURE) names_set(m.aoUvSetIndex);
            // the opacity slot only feeds the alpha channel, which the G-buffer does not store; the rasteriser's alpha test reads UV set 0 as the reference's does
        }
    }
    t.uvSets = uvSets;
    t.hasVertexColors = false;
    for (const brmi_per_mesh& pm : hs.perMesh) if (pm.vertexFlags & 1u) t.hasVertexColors = true;       // VERTEX_COLORS (BR/include/Mesh/VertexFlags.h)
    if (hs.openpbrMaterials.size() > 65536u) return refuse(msg, BRMI_ERR_CAPACITY, "brmi_set_scene: %u OpenPBR material records; the shading pass folds 66 KB of table rows per record and takes at most 65536", (uint32_t)hs.openpbrMaterials.size());
    if (t.hasTextures && !hs.textureTables)
        return refuse(msg, BRMI_ERR_INVALID, "brmi_set_scene: materials sample textures but the texture / sampler tables or the sRGB decode table are missing");
    return BRMI_OK;
}

// Cross references the kernels follow unchecked: validated once here, on the host copies (a bad index is an error message, not a
// GPU fault).  Page contents (headers, descriptors, streams inside the slabs) are NOT walked: they are the builder's contract.
inline int validate_references(const HostScene& hs, std::string& msg) {
    const auto& insts = hs.perMeshInstance; const auto& pms = hs.perMesh; const auto& mats = hs.materials; const auto& pmap = hs.groupPageMap; const auto& md = hs.meshMetadata; const auto& segs = hs.lodSegments;
    for (size_t i = 0; i < hs.activeDraws.size(); i++) if (hs.activeDraws[i] >= insts.size()) return refuse(msg, BRMI_ERR_INVALID, "activeDraws[%zu] = %u: no such mesh instance", i, hs.activeDraws[i]);
    for (size_t i = 0; i < insts.size(); i++) {
        if (insts[i].perMeshBufferIndex >= pms.size()) return refuse(msg, BRMI_ERR_INVALID, "mesh instance %zu: perMeshBufferIndex %u out of range", i, insts[i].perMeshBufferIndex);
        if (insts[i].perObjectBufferIndex >= hs.perObjectCount) return refuse(msg, BRMI_ERR_INVALID, "mesh instance %zu: perObjectBufferIndex %u out of range", i, insts[i].perObjectBufferIndex);
        if ((pms[insts[i].perMeshBufferIndex].vertexFlags & BRMI_VERTEX_SKINNED) && insts[i].skinningInstanceSlot != 0xFFFFFFFFu &&
            ((uint64_t)insts[i].skinningInstanceSlot + 1u) * 64u > hs.skinningMatrixCount)
            return refuse(msg, BRMI_ERR_INVALID, "mesh instance %zu: skinning slot %u lies outside the skinning matrix buffer", i, insts[i].skinningInstanceSlot);
    }
    for (size_t i = 0; i < pms.size(); i++) if (pms[i].materialDataIndex >= mats.size()) return refuse(msg, BRMI_ERR_INVALID, "mesh %zu: materialDataIndex %u out of range", i, pms[i].materialDataIndex);
    for (size_t i = 0; i < mats.size(); i++) if (mats[i].openPBRMaterialDataIndex >= hs.openpbrMaterials.size()) return refuse(msg, BRMI_ERR_INVALID, "material %zu: openPBRMaterialDataIndex %u out of range", i, mats[i].openPBRMaterialDataIndex);
    for (size_t i = 0; i < pmap.size(); i++) {
        if (pmap[i].slabDescriptorIndex >= hs.slabs.size()) return refuse(msg, BRMI_ERR_INVALID, "page map entry %zu: slab %u out of range", i, pmap[i].slabDescriptorIndex);
        if (pmap[i].slabByteOffset % BRMI_PAGE_SIZE) return refuse(msg, BRMI_ERR_INVALID, "page map entry %zu: offset %u is not a page boundary", i, pmap[i].slabByteOffset);
    }
    for (size_t m = 0; m < md.size(); m++) if (md[m].groupsBase > hs.lodGroups.size() || md[m].segmentsBase > segs.size() || md[m].pageMapBase > pmap.size()) return refuse(msg, BRMI_ERR_INVALID, "mesh metadata %zu: base index out of range", m);
    for (size_t i = 0; i < hs.clodOffsets.size(); i++) if (hs.clodOffsets[i].clodMeshMetadataIndex >= md.size()) return refuse(msg, BRMI_ERR_INVALID, "instance %zu: bad mesh metadata index", i);
    // segments -> pages and refined groups, relative to the mesh that owns them (a mesh's segments end where the next mesh's begin)
    std::vector<uint32_t> order(md.size());
    for (size_t m = 0; m < md.size(); m++) order[m] = (uint32_t)m;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return md[a].segmentsBase < md[b].segmentsBase; });
    for (size_t k = 0; k < order.size(); k++) {
        const brmi_clod_mesh_metadata& mm = md[order[k]];
        const size_t segEnd = k + 1 < order.size() ? md[order[k + 1]].segmentsBase : segs.size();
        for (size_t si = mm.segmentsBase; si < segEnd; si++) {
            if ((uint64_t)mm.pageMapBase + segs[si].pageIndex >= pmap.size()) return refuse(msg, BRMI_ERR_INVALID, "segment %zu: page %u lies outside the group page map", si, segs[si].pageIndex);
            if (segs[si].refinedGroup >= 0 && (uint64_t)mm.groupsBase + (uint32_t)segs[si].refinedGroup >= hs.lodGroups.size()) return refuse(msg, BRMI_ERR_INVALID, "segment %zu: refined group %d out of range", si, segs[si].refinedGroup);
        }
    }
    return BRMI_OK;
}

// per mesh: walk the BVH, collect the segments its leaves reference, depth of the tree and width of its levels; then the bit base of every instance
inline int build_rank_tables(const HostScene& hs, SceneTables& t, std::string& msg) {
    const auto& md = hs.meshMetadata; const auto& nodes = hs.lodNodes; const auto& segs = hs.lodSegments;
    t.segPrefix.assign(segs.size(), 0);
    std::vector<uint32_t> meshBits(md.size(), 0);
    t.maxDepth = 1;
    t.maxLevelWidth = 1; t.minLevelWidth = 0xFFFFFFFFu; t.meshLevelWidth.assign(md.size(), 1u);
    t.spillLevels = 0;
    std::vector<uint32_t> levelWidth;
    std::vector<std::pair<uint32_t, uint32_t>> stack;
    for (size_t m = 0; m < md.size(); m++) {
        uint32_t segCount = 0;
        levelWidth.assign(66, 0);
        stack.clear(); stack.push_back({md[m].rootNode, 1});
        while (!stack.empty()) {
            auto [n, d] = stack.back(); stack.pop_back();
            if ((uint64_t)md[m].lodNodesBase + n >= nodes.size()) return refuse(msg, BRMI_ERR_INVALID, "mesh %zu: node %u out of range", m, n);
            const brmi_lod_node& nd = nodes[md[m].lodNodesBase + n];
            t.maxDepth = std::max(t.maxDepth, d);
            if (d < levelWidth.size()) t.meshLevelWidth[m] = std::max(t.meshLevelWidth[m], ++levelWidth[d]);
            if (nd.isLeaf != BRMI_NODE_INTERNAL) {
                // a leaf names its group and (countMinusOne - 1) the group that refines it: the traversal reads both records unchecked
                if ((uint64_t)md[m].groupsBase + nd.ownerGroupId >= hs.lodGroups.size()) return refuse(msg, BRMI_ERR_INVALID, "mesh %zu: leaf node %u names group %u, which does not exist", m, n, nd.ownerGroupId);
                if (nd.countMinusOne != 0u && (uint64_t)md[m].groupsBase + (nd.countMinusOne - 1u) >= hs.lodGroups.size()) return refuse(msg, BRMI_ERR_INVALID, "mesh %zu: leaf node %u names refined group %u, which does not exist", m, n, nd.countMinusOne - 1u);
                segCount = std::max(segCount, nd.indexOrOffset + 1); continue;
            }
            if (d > 64) return refuse(msg, BRMI_ERR_INVALID, "mesh %zu: BVH deeper than 64 levels", m);
            const uint32_t cc = std::min(nd.countMinusOne + 1u, BRMI_BVH_MAX_CHILDREN);
            for (uint32_t k = 0; k < cc; k++) stack.push_back({nd.indexOrOffset + k, d + 1});
        }
        uint64_t run = 0;
        for (uint32_t s = 0; s < segCount; s++) {
            const size_t gi = (size_t)md[m].segmentsBase + s;
            if (gi >= segs.size()) return refuse(msg, BRMI_ERR_INVALID, "mesh %zu: segment %u out of range", m, s);
            t.segPrefix[gi] = (uint32_t)run; run += segs[gi].meshletCount;
        }
        if (run > 0xFFFFFFFFull) return refuse(msg, BRMI_ERR_CAPACITY, "mesh %zu has too many meshlets", m);
        meshBits[m] = (uint32_t)run;
        t.maxLevelWidth = std::max(t.maxLevelWidth, t.meshLevelWidth[m]); t.minLevelWidth = std::min(t.minLevelWidth, t.meshLevelWidth[m]);
        if (t.meshLevelWidth[m] > t.spillWidth) {
            // a mesh too wide for the LDS walk: the walk hands its frontier to the level kernels at the first level that holds more than 128 nodes
            // (brmi_cull.hip, spill mode) -- never above the first level that CAN hold that many; what is left below bounds the level launches
            uint32_t depth = 1, first = 0;
            for (uint32_t d = 1; d < levelWidth.size(); d++) { if (levelWidth[d]) depth = d; if (!first && levelWidth[d] > 128u) first = d; }
            if (first) t.spillLevels = std::max(t.spillLevels, depth - first + 1u);
        }
    }
    t.instanceBitBase.assign(hs.clodOffsets.size(), 0);
    uint64_t bits = 0;
    for (size_t i = 0; i < hs.clodOffsets.size(); i++) {      // (validate_references has looked at every clodMeshMetadataIndex)
        t.instanceBitBase[i] = (uint32_t)bits; bits += meshBits[hs.clodOffsets[i].clodMeshMetadataIndex];
        if (bits > 0xFFFFFFF0ull) return refuse(msg, BRMI_ERR_CAPACITY, "scene exceeds 2^32 (instance, meshlet) pairs");
    }
    t.totalBits = bits;
    return BRMI_OK;
}

// flat traversal tables: the BVH of a mesh with at most 8192 nodes, breadth-first, with what its leaves' groups and segments say folded in.
// After build_rank_tables (its walk has refused every node and group index out of range, and made segPrefix and instanceBitBase).
inline int build_flat_tables(const HostScene& hs, bool flatOn, uint32_t maxBvhLevels, SceneTables& t, std::string& msg) {
    const auto& md = hs.meshMetadata; const auto& nodes = hs.lodNodes; const auto& segs = hs.lodSegments; const auto& groups = hs.lodGroups;
    t.flatNodes.clear(); t.flatLeaves.clear(); t.flatMaxDepth = 1;
    std::vector<uint32_t> flatBase(md.size(), 0), flatCount(md.size(), 0);
    std::vector<std::pair<uint32_t, uint32_t>> bfs;      // (node id, parent position)
    for (size_t m = 0; flatOn && m < md.size(); m++) {
        bfs.clear(); bfs.push_back({md[m].rootNode, 0u});
        bool fits = true;
        for (size_t k = 0; k < bfs.size() && fits; k++) {
            const brmi_lod_node& nd = nodes[md[m].lodNodesBase + bfs[k].first];
            if (nd.isLeaf != BRMI_NODE_INTERNAL) continue;
            const uint32_t cc = std::min(nd.countMinusOne + 1u, BRMI_BVH_MAX_CHILDREN);
            for (uint32_t c = 0; c < cc; c++) { bfs.push_back({nd.indexOrOffset + c, (uint32_t)k}); if (bfs.size() > 8192) { fits = false; break; } }
        }
        if (!fits) continue;
        flatBase[m] = (uint32_t)t.flatNodes.size(); flatCount[m] = (uint32_t)bfs.size();
        // (breadth-first: the children of a node are pushed together, so they sit side by side; position of the first and depth of every node)
        std::vector<uint32_t> firstChild(bfs.size(), 0u), childCount(bfs.size(), 0u), depthOf(bfs.size(), 1u);
        uint32_t meshDepth = 1u;
        for (size_t k = 1; k < bfs.size(); k++) { const uint32_t par = bfs[k].second; if (childCount[par]++ == 0u) firstChild[par] = (uint32_t)k; depthOf[k] = depthOf[par] + 1u; meshDepth = std::max(meshDepth, depthOf[k]); }
        // the level-synchronous traversal keeps a frontier size per level in counters[CNT_FRONTIER0 + level] (96 words up to the stripe statistics) and launches a kernel per
        // level: a hierarchy deeper than that, or than the configured level bound, is left to the level walk
        if (meshDepth > std::min<uint32_t>(std::max(1u, maxBvhLevels), CNT_STRIPES - CNT_FRONTIER0 - 1u)) { flatCount[m] = 0; continue; }
        t.flatMaxDepth = std::max(t.flatMaxDepth, meshDepth);
        for (size_t k = 0; k < bfs.size(); k++) {
            const brmi_lod_node& nd = nodes[md[m].lodNodesBase + bfs[k].first];
            FlatNode f{}; FlatLeaf l{};
            f.children = firstChild[k] | (childCount[k] << 16);
            std::memcpy(f.cull, nd.cullCenterAndRadius, 16); std::memcpy(f.lod, nd.lodCenterAndRadius, 16); f.maxQuadricError = nd.maxQuadricError;
            f.nodeId = bfs[k].first; f.info = bfs[k].second << 8;
            if (nd.isLeaf == BRMI_NODE_INTERNAL) f.info |= 1u;
            else {
                const brmi_lod_group& g = groups[md[m].groupsBase + nd.ownerGroupId];
                std::memcpy(l.group, g.centerAndRadius, 16); l.ownerGlobal = md[m].groupsBase + nd.ownerGroupId;
                if (nd.countMinusOne != 0u) { const brmi_lod_group& cg = groups[md[m].groupsBase + (nd.countMinusOne - 1u)]; std::memcpy(l.child, cg.centerAndRadius, 16); l.childParentError = cg.maxParentError; l.childGlobal = md[m].groupsBase + (nd.countMinusOne - 1u); f.info |= 1u << 1; }
                // (build_rank_tables has refused every segment up to the highest a leaf names, except for a leaf that names segment 2^32 - 1: there its count wraps to 0)
                const size_t si = (size_t)md[m].segmentsBase + nd.indexOrOffset;
                if (si >= segs.size()) return refuse(msg, BRMI_ERR_INVALID, "mesh %zu: leaf node %u names segment %u, which does not exist", m, bfs[k].first, nd.indexOrOffset);
                if (segs[si].meshletCount != 0u) f.info |= 1u << 2;
                if (segs[si].meshletCount > 0xFFFFu || segs[si].firstMeshletInPage > 0xFFFFu) { flatCount[m] = 0; break; }      // (the bucket record packs both in 16 bits; leave such a mesh to the level walk)
                f.ownerGroup = nd.ownerGroupId; f.segFirstCount = segs[si].firstMeshletInPage | (segs[si].meshletCount << 16);
                f.pageMapIndex = md[m].pageMapBase + segs[si].pageIndex; f.firstBitRel = t.segPrefix[si];
            }
            t.flatNodes.push_back(f); t.flatLeaves.push_back(l);
        }
        if (flatCount[m] == 0) { t.flatNodes.resize(flatBase[m]); t.flatLeaves.resize(flatBase[m]); }
    }
    t.anyWideFlat = false; t.allMeshesFlat = flatOn;
    for (size_t m = 0; m < md.size(); m++) { if (flatCount[m] > 256u) t.anyWideFlat = true; if (flatCount[m] == 0u) t.allMeshesFlat = false; }
    t.instanceWalk.assign(hs.clodOffsets.size(), InstanceWalk{0, 0, 0, 0});
    for (size_t i = 0; i < hs.clodOffsets.size(); i++) {      // (validate_references has looked at every perMeshBufferIndex)
        const uint32_t m = hs.clodOffsets[i].clodMeshMetadataIndex;
        const bool skinned = (hs.perMesh[hs.perMeshInstance[i].perMeshBufferIndex].vertexFlags & BRMI_VERTEX_SKINNED) != 0;
        t.instanceWalk[i] = InstanceWalk{flatBase[m], flatCount[m], t.instanceBitBase[i], skinned ? 1u : 0u};
    }
    return BRMI_OK;
}

// Round 6, the draw list: every resident page of the page map, and where its meshlets' boxes start in the side table (k_meshlet_boxes fills it in brmi_setup).
// A page's meshlet count is the first word of its header (the builder's contract; one small read per distinct resident page, not per page-map entry or frame).
inline int build_page_table(const HostScene& hs, bool boxesOn, const PageHeaderReader& readMeshletCount, SceneTables& t) {
    const auto& pmap = hs.groupPageMap;
    t.pageRefs.clear(); t.totalBoxes = 0;
    t.pageBoxBase.assign(std::max<size_t>(1, hs.slabs.size()) * 1024u, 0xFFFFFFFFu);
    for (size_t i = 0; boxesOn && i < pmap.size(); i++) {
        const uint32_t slab = pmap[i].slabDescriptorIndex, page = pmap[i].slabByteOffset / BRMI_PAGE_SIZE;
        if (slab == 0u || page >= 1024u || !hs.slabs[slab]) continue;      // not resident (or beyond the 10 page bits of the packed cluster: such a page is never named)
        uint32_t& base = t.pageBoxBase[(size_t)slab * 1024u + page];
        if (base != 0xFFFFFFFFu) continue;                                  // several groups share a page
        uint32_t meshlets = 0;
        if (int rc = readMeshletCount(slab, pmap[i].slabByteOffset, &meshlets)) return rc;
        meshlets = std::min(meshlets, (BRMI_PAGE_SIZE - 64u) / 64u);
        if ((uint64_t)t.totalBoxes + meshlets > 0x7FFFFFFFull) break;
        base = t.totalBoxes;
        t.pageRefs.push_back(PageRef{slab, pmap[i].slabByteOffset, base, meshlets});
        t.totalBoxes += meshlets;
    }
    return BRMI_OK;
}

// Everything above, in the order whose first refusal a caller sees.  A refusal leaves `t` partly written and its text in `msg` (a failed page read: what the reader reports).
inline int analyse_scene(const HostScene& hs, bool flatOn, uint32_t maxBvhLevels, bool boxesOn, const PageHeaderReader& readMeshletCount, SceneTables& t, std::string& msg) {
    if (int rc = classify_materials(hs, t, msg)) return rc;
    if (int rc = validate_references(hs, msg)) return rc;
    if (int rc = build_rank_tables(hs, t, msg)) return rc;
    if (int rc = build_flat_tables(hs, flatOn, maxBvhLevels, t, msg)) return rc;
    return build_page_table(hs, boxesOn, readMeshletCount, t);
}

}  // namespace brmi
#endif
