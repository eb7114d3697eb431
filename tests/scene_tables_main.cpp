// scene_tables_main.cpp -- brmi_scene_tables.h (what brmi_set_scene derives from a scene) run on the host, for tests/test_scene_tables_cpu.py,
// which builds this with the address and undefined-behaviour sanitizers.  Links libbrmi_scene.so only.
//   tables  OUTDIR FEATURES SKINNED1024   analyse the generated scene Scene("tiny", 128, 72, point_lights=1, lod_levels=2, material_features=FEATURES,
//                                         skinned_fraction=SKINNED1024/1024); the tables as raw arrays and scalars.json into OUTDIR
//   refuse  NAME                          one named corruption of that scene (or a hand-made scene); prints the status and the message
//   shape   NAME                          a hand-made hierarchy; prints the scalars
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../basicrenderer_amd/csrc/brmi_scene_tables.h"
#include "brmi_scene.h"

using namespace brmi;

static int read_page_header(const HostScene& hs, uint32_t slab, uint32_t byteOffset, uint32_t* meshlets) {
    std::memcpy(meshlets, hs.slabs[slab] + byteOffset, 4);
    return BRMI_OK;
}

template <typename T>
static void take(const brmi_scene* s, uint32_t id, std::vector<T>& dst) {
    const void* ptr = nullptr; uint64_t bytes = 0; uint32_t count = 0;
    if (brmi_scene_array(s, id, &ptr, &bytes, &count) != 0 || bytes != (uint64_t)count * sizeof(T)) { std::fprintf(stderr, "brmi_scene_array(%u) failed\n", id); std::exit(2); }
    dst.resize(count);
    if (count) std::memcpy(dst.data(), ptr, bytes);
}

static brmi_scene* g_scene = nullptr;      // alive until main returns: HostScene::slabs points into it
static HostScene generated_scene(uint32_t features, uint32_t skinned1024) {
    brmi_scene_params prm{};
    prm.preset = BRMI_PRESET_TINY; prm.width = 128; prm.height = 72; prm.numPointLights = 1; prm.withDirectionalLight = 1; prm.lodLevels = 2;
    prm.sizeScale = 1.0f; prm.detail = 1.0f; prm.materialFeatures = features; prm.skinnedFraction1024 = skinned1024; prm.lodBuilder = BRMI_LOD_BUILDER_QUADTREE;
    brmi_scene* s = g_scene = brmi_scene_create(&prm);
    if (!s) { std::fprintf(stderr, "brmi_scene_create failed\n"); std::exit(2); }
    HostScene hs;
    take(s, BRMI_ARR_CLOD_MESH_METADATA, hs.meshMetadata); take(s, BRMI_ARR_CLOD_OFFSETS, hs.clodOffsets); take(s, BRMI_ARR_LOD_NODES, hs.lodNodes);
    take(s, BRMI_ARR_LOD_SEGMENTS, hs.lodSegments); take(s, BRMI_ARR_LOD_GROUPS, hs.lodGroups); take(s, BRMI_ARR_GROUP_PAGE_MAP, hs.groupPageMap);
    take(s, BRMI_ARR_PER_MESH, hs.perMesh); take(s, BRMI_ARR_PER_MESH_INSTANCE, hs.perMeshInstance); take(s, BRMI_ARR_MATERIALS, hs.materials);
    take(s, BRMI_ARR_OPENPBR_MATERIALS, hs.openpbrMaterials); take(s, BRMI_ARR_ACTIVE_DRAWS, hs.activeDraws);
    const void* ptr = nullptr; uint64_t bytes = 0; uint32_t count = 0, textures = 0, samplers = 0, srgb = 0;
    brmi_scene_array(s, BRMI_ARR_PER_OBJECT, &ptr, &bytes, &hs.perObjectCount);
    brmi_scene_array(s, BRMI_ARR_SKINNING_MATRICES, &ptr, &bytes, &hs.skinningMatrixCount);
    brmi_scene_array(s, BRMI_ARR_TEXTURE_DESCS, &ptr, &bytes, &textures); brmi_scene_array(s, BRMI_ARR_SAMPLER_DESCS, &ptr, &bytes, &samplers); brmi_scene_array(s, BRMI_ARR_SRGB_TO_LINEAR, &ptr, &bytes, &srgb);
    hs.textureTables = textures != 0 && samplers != 0 && srgb != 0;
    count = brmi_scene_slab_count(s);
    hs.slabs.assign(count + 1u, nullptr);      // entry 0: "not resident"
    for (uint32_t i = 1; i <= count; i++) { brmi_scene_slab(s, i, &ptr, &bytes); hs.slabs[i] = static_cast<const uint8_t*>(ptr); }
    return hs;
}

// ---- hand-made scenes: one mesh of one group and one segment (4 meshlets in page 0 of slab 1), one instance, under a root with two leaves ----
static std::vector<uint32_t> g_slab;     // two pages; a page header has its meshletCount first

static brmi_lod_node leaf(uint32_t segment) { brmi_lod_node n{}; n.isLeaf = BRMI_NODE_SEGMENT_LEAF; n.indexOrOffset = segment; return n; }
static brmi_lod_node internal(uint32_t firstChild, uint32_t children) { brmi_lod_node n{}; n.isLeaf = BRMI_NODE_INTERNAL; n.indexOrOffset = firstChild; n.countMinusOne = children - 1u; return n; }

static HostScene base_scene() {
    HostScene hs;
    brmi_openpbr_material_info op{}; for (int k = 0; k < 12; k++) op.textureBindings[k] = 0xFFFFFFFFu;
    hs.openpbrMaterials.push_back(op);
    hs.materials.push_back(brmi_material_info{});
    hs.perMesh.push_back(brmi_per_mesh{});
    brmi_per_mesh_instance inst{}; inst.skinningInstanceSlot = 0xFFFFFFFFu;
    hs.perMeshInstance.push_back(inst); hs.clodOffsets.push_back(brmi_mesh_instance_clod_offsets{0u});
    hs.perObjectCount = 1; hs.activeDraws.push_back(0u);
    hs.meshMetadata.push_back(brmi_clod_mesh_metadata{});
    hs.lodGroups.push_back(brmi_lod_group{});
    hs.lodSegments.push_back(brmi_lod_segment{-1, 0u, 4u, 0u});
    hs.groupPageMap.push_back(brmi_group_page_map_entry{1u, 0u});
    g_slab.assign(2 * BRMI_PAGE_SIZE / 4, 0u); g_slab[0] = 4u; g_slab[BRMI_PAGE_SIZE / 4] = 7u;
    hs.slabs = {nullptr, reinterpret_cast<const uint8_t*>(g_slab.data())};
    hs.lodNodes = {internal(1, 2), leaf(0), leaf(0)};
    return hs;
}
// a complete 8-ary tree of `depth` levels, breadth-first (node k's children: 8 k + 1 ..), the last level leaves of segment 0
static std::vector<brmi_lod_node> full_tree(uint32_t depth) {
    std::vector<brmi_lod_node> nodes;
    size_t levelFirst = 0, levelCount = 1;
    for (uint32_t d = 1; d <= depth; d++) {
        for (size_t k = levelFirst; k < levelFirst + levelCount; k++) nodes.push_back(d == depth ? leaf(0) : internal((uint32_t)(8 * k + 1), 8));
        levelFirst += levelCount; levelCount *= 8;
    }
    return nodes;
}
// a second mesh with nodes, segments and group of its own behind the first one's, and an instance of it
static void add_mesh(HostScene& hs, const std::vector<brmi_lod_node>& nodes, const brmi_lod_segment& seg) {
    brmi_clod_mesh_metadata md{}; md.groupsBase = (uint32_t)hs.lodGroups.size(); md.segmentsBase = (uint32_t)hs.lodSegments.size(); md.lodNodesBase = (uint32_t)hs.lodNodes.size();
    hs.lodNodes.insert(hs.lodNodes.end(), nodes.begin(), nodes.end()); hs.lodSegments.push_back(seg); hs.lodGroups.push_back(brmi_lod_group{});
    hs.clodOffsets.push_back(brmi_mesh_instance_clod_offsets{(uint32_t)hs.meshMetadata.size()}); hs.perMeshInstance.push_back(hs.perMeshInstance[0]);
    hs.meshMetadata.push_back(md);
}

static void poke(void* base, size_t elemBytes, size_t elem, size_t word, uint32_t value) { std::memcpy(static_cast<char*>(base) + elem * elemBytes + word * 4, &value, 4); }

struct Case { HostScene hs; uint32_t maxBvhLevels = 64; };

static bool named_case(const std::string& name, Case& c) {
    HostScene& hs = c.hs;
    auto gen = [&](uint32_t features = 0) { hs = generated_scene(features, 0); };
    auto first_leaf = [&]() { for (size_t i = 0; i < hs.lodNodes.size(); i++) if (hs.lodNodes[i].isLeaf == BRMI_NODE_SEGMENT_LEAF) return i; std::exit(2); };
    // the corruptions of tests/test_parity_gpu.py: test_dangling_scene_indices_are_refused, test_missing_texture_table_is_refused
    if (name == "activeDraws") { gen(); hs.activeDraws[0] = 1u << 20; }
    else if (name == "perMeshBufferIndex") { gen(); hs.perMeshInstance[0].perMeshBufferIndex = 9999; }
    else if (name == "perObjectBufferIndex") { gen(); hs.perMeshInstance[1].perObjectBufferIndex = 9999; }
    else if (name == "materialDataIndex") { gen(); hs.perMesh[0].materialDataIndex = 9999; }
    else if (name == "slab") { gen(); hs.groupPageMap[0].slabDescriptorIndex = 77; }
    else if (name == "pageBoundary") { gen(); hs.groupPageMap[0].slabByteOffset = 12345; }
    else if (name == "segmentPage") { gen(); hs.lodSegments[0].pageIndex = 9999; }
    else if (name == "clodOffsets") { gen(); hs.clodOffsets[0].clodMeshMetadataIndex = 9999; }
    else if (name == "leafGroup") { gen(); hs.lodNodes[first_leaf()].ownerGroupId = 1u << 24; }
    else if (name == "leafRefinedGroup") { gen(); hs.lodNodes[first_leaf()].countMinusOne = 1u << 24; }
    else if (name == "openPBRMaterialDataIndex") { gen(); poke(hs.materials.data(), sizeof(brmi_material_info), 0, 60, 9999); }
    else if (name == "textureTable") { gen(8); hs.textureTables = false; }
    // the refusals no generated scene reaches
    else if (name == "nodeOutOfRange") { hs = base_scene(); hs.lodNodes[0].indexOrOffset = 1000; }
    else if (name == "segmentOutOfRange") { hs = base_scene(); hs.lodNodes[2].indexOrOffset = 5; }
    else if (name == "segmentWraps") { hs = base_scene(); hs.lodNodes[2].indexOrOffset = 0xFFFFFFFFu; }      // its count wraps to 0: the flat tables' own check
    else if (name == "deeperThan64") { hs = base_scene(); hs.lodNodes.clear(); for (uint32_t k = 0; k < 65; k++) hs.lodNodes.push_back(internal(k + 1, 1)); hs.lodNodes.push_back(leaf(0)); }
    else if (name == "skinningSlot") { hs = base_scene(); hs.perMesh[0].vertexFlags = BRMI_VERTEX_SKINNED; hs.perMeshInstance[0].skinningInstanceSlot = 3; hs.skinningMatrixCount = 255; }
    else if (name == "openpbrRecords") { hs = base_scene(); hs.openpbrMaterials.resize(65537, hs.openpbrMaterials[0]); }
    else if (name == "meshMeshlets") { hs = base_scene(); hs.lodSegments[0].meshletCount = 0x80000000u; hs.lodSegments.push_back(hs.lodSegments[0]); hs.lodNodes[2].indexOrOffset = 1; }
    else if (name == "instancePairs") { hs = base_scene(); hs.lodSegments[0].meshletCount = 0x80000000u; hs.clodOffsets.push_back(hs.clodOffsets[0]); hs.perMeshInstance.push_back(hs.perMeshInstance[0]); }
    // hand-made hierarchies: where a mesh leaves the flat tables, the spill path, shared pages
    else if (name == "plain") { hs = base_scene(); }
    else if (name == "tooManyNodes") { hs = base_scene(); hs.lodNodes = full_tree(6); }                     // 37449 nodes, levels of 1 .. 32768
    else if (name == "wideLevel") { hs = base_scene(); hs.lodNodes = full_tree(5); }                        // 4681 nodes, levels of 1, 8, 64, 512, 4096
    else if (name == "bigSegment") { hs = base_scene(); add_mesh(hs, {internal(1, 2), leaf(0), leaf(0)}, brmi_lod_segment{-1, 0u, 0x10000u, 0u}); }
    else if (name == "deepForLevelBound") { hs = base_scene(); hs.lodNodes = {internal(1, 1), internal(2, 1), internal(3, 1), leaf(0)}; c.maxBvhLevels = 3; }
    else if (name == "deepWithinLevelBound") { hs = base_scene(); hs.lodNodes = {internal(1, 1), internal(2, 1), internal(3, 1), leaf(0)}; c.maxBvhLevels = 4; }
    else if (name == "sharedPage") { hs = base_scene(); hs.groupPageMap.push_back(hs.groupPageMap[0]); hs.groupPageMap.push_back(brmi_group_page_map_entry{1u, BRMI_PAGE_SIZE}); hs.groupPageMap.push_back(brmi_group_page_map_entry{0u, 0u}); }
    else return false;
    return true;
}

template <typename T>
static void dump(const std::string& dir, const char* name, const std::vector<T>& v) {
    FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
    if (!f || (v.size() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size())) { std::fprintf(stderr, "cannot write %s\n", name); std::exit(2); }
    std::fclose(f);
}

static void print_scalars(FILE* f, const SceneTables& t) {
    std::fprintf(f, "{\"hasCoat\": %d, \"hasFuzz\": %d, \"hasAlphaTest\": %d, \"hasTextures\": %d, \"hasParallax\": %d, \"hasVertexColors\": %d, \"uvSets\": %u,\n", t.hasCoat, t.hasFuzz, t.hasAlphaTest,
                 t.hasTextures, t.hasParallax, t.hasVertexColors, t.uvSets);
    std::fprintf(f, " \"totalBits\": %llu, \"maxDepth\": %u, \"maxLevelWidth\": %u, \"minLevelWidth\": %u, \"spillLevels\": %u,\n", (unsigned long long)t.totalBits, t.maxDepth, t.maxLevelWidth, t.minLevelWidth, t.spillLevels);
    std::fprintf(f, " \"flatNodes\": %zu, \"flatLeaves\": %zu, \"flatMaxDepth\": %u, \"anyWideFlat\": %d, \"allMeshesFlat\": %d, \"pageRefs\": %zu, \"totalBoxes\": %u, \"flatCounts\": [", t.flatNodes.size(),
                 t.flatLeaves.size(), t.flatMaxDepth, t.anyWideFlat, t.allMeshesFlat, t.pageRefs.size(), t.totalBoxes);
    for (size_t i = 0; i < t.instanceWalk.size(); i++) std::fprintf(f, "%s%u", i ? ", " : "", t.instanceWalk[i].flatCount);
    std::fprintf(f, "]}\n");
}

static int run(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    SceneTables t; std::string msg;
    if (mode == "tables" && argc == 5) {
        const std::string dir = argv[2];
        const HostScene hs = generated_scene((uint32_t)std::strtoul(argv[3], nullptr, 0), (uint32_t)std::strtoul(argv[4], nullptr, 0));
        const PageHeaderReader reader = [&](uint32_t slab, uint32_t off, uint32_t* n) { return read_page_header(hs, slab, off, n); };
        const int rc = analyse_scene(hs, true, 64, true, reader, t, msg);
        if (rc) { std::fprintf(stderr, "analyse_scene: %d %s\n", rc, msg.c_str()); return 1; }
        dump(dir, "segPrefix.u32", t.segPrefix); dump(dir, "instanceBitBase.u32", t.instanceBitBase); dump(dir, "meshLevelWidth.u32", t.meshLevelWidth);
        dump(dir, "flatNodes.bin", t.flatNodes); dump(dir, "flatLeaves.bin", t.flatLeaves); dump(dir, "instanceWalk.u32", t.instanceWalk);
        dump(dir, "pageRefs.u32", t.pageRefs); dump(dir, "pageBoxBase.u32", t.pageBoxBase);
        FILE* f = std::fopen((dir + "/scalars.json").c_str(), "w");
        if (!f) return 2;
        print_scalars(f, t); std::fclose(f);
        // the page table once more without the draw list's boxes (a pass without occlusion culling, or BRMI_TUNING hold_clusters=0)
        if (build_page_table(hs, false, reader, t)) return 1;
        dump(dir, "pageRefs_off.u32", t.pageRefs); dump(dir, "pageBoxBase_off.u32", t.pageBoxBase);
        std::printf("%u\n", t.totalBoxes);
        return 0;
    }
    Case c;
    if ((mode == "refuse" || mode == "shape") && argc == 3 && named_case(argv[2], c)) {
        const PageHeaderReader reader = [&](uint32_t slab, uint32_t off, uint32_t* n) { return read_page_header(c.hs, slab, off, n); };
        const int rc = analyse_scene(c.hs, true, c.maxBvhLevels, true, reader, t, msg);
        if (mode == "refuse") { std::printf("%d\n%s\n", rc, msg.c_str()); return 0; }
        if (rc) { std::fprintf(stderr, "analyse_scene: %d %s\n", rc, msg.c_str()); return 1; }
        print_scalars(stdout, t);
        return 0;
    }
    std::fprintf(stderr, "usage: %s tables OUTDIR FEATURES SKINNED1024 | refuse NAME | shape NAME\n", argv[0]);
    return 2;
}

int main(int argc, char** argv) {
    const int rc = run(argc, argv);
    if (g_scene) brmi_scene_destroy(g_scene);
    return rc;
}
