// user_materials_main.cpp -- a scene of brmi_scene_create_from_meshes_with_materials put through analyse_scene (brmi_scene_tables.h) on the host, for
// tests/test_gltf_materials_cpu.py.  Links libbrmi_scene.so only.
//   analyse DIR [noTables]   DIR holds what the test wrote from gltf.load_gltf_materials: materials.bin (brmi_material_info[]), samplers.bin
//                            (brmi_sampler_desc[]), textures.bin (per texture: width, height, format as uint32, then width x height RGBA8 texels).  The
//                            geometry is the fixture's: two quads, the second with a second UV set.  Prints the status, the message and the scalars;
//                            `noTables`: the same scene analysed as if its texture tables had not been bound.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../basicrenderer_amd/csrc/brmi_scene_tables.h"
#include "brmi_scene.h"

using namespace brmi;

static std::vector<uint8_t> slurp(const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); std::exit(2); }
    std::vector<uint8_t> v; uint8_t buf[4096]; size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}
template <typename T>
static void take(const brmi_scene* s, uint32_t id, std::vector<T>& dst) {
    const void* ptr = nullptr; uint64_t bytes = 0; uint32_t count = 0;
    if (brmi_scene_array(s, id, &ptr, &bytes, &count) != 0 || bytes != (uint64_t)count * sizeof(T)) { std::fprintf(stderr, "brmi_scene_array(%u) failed\n", id); std::exit(2); }
    dst.resize(count);
    if (count) std::memcpy(dst.data(), ptr, bytes);
}

int main(int argc, char** argv) {
    if (argc < 3 || std::string(argv[1]) != "analyse") { std::fprintf(stderr, "usage: %s analyse DIR [noTables]\n", argv[0]); return 2; }
    const std::string dir = argv[2];
    const bool noTables = argc > 3 && std::string(argv[3]) == "noTables";
    const std::vector<uint8_t> mats = slurp(dir + "/materials.bin"), samp = slurp(dir + "/samplers.bin"), tex = slurp(dir + "/textures.bin");
    if (mats.size() % sizeof(brmi_material_info) || samp.size() % sizeof(brmi_sampler_desc)) { std::fprintf(stderr, "table sizes\n"); return 2; }
    std::vector<brmi_material_info> materials(mats.size() / sizeof(brmi_material_info));
    std::memcpy(materials.data(), mats.data(), mats.size());
    std::vector<brmi_sampler_desc> samplers(samp.size() / sizeof(brmi_sampler_desc));
    std::memcpy(samplers.data(), samp.data(), samp.size());
    std::vector<brmi_texture_desc> textures;
    for (size_t at = 0; at + 12 <= tex.size();) {
        uint32_t head[3]; std::memcpy(head, tex.data() + at, 12);
        brmi_texture_desc d{};
        d.width = head[0]; d.height = head[1]; d.format = head[2]; d.texels = tex.data() + at + 12;
        for (uint32_t m = d.width > d.height ? d.width : d.height; m; m >>= 1) d.mipCount++;
        textures.push_back(d);
        at += 12 + (size_t)d.width * d.height * 4;
        if (at > tex.size()) { std::fprintf(stderr, "textures.bin is short\n"); return 2; }
    }
    const float quad0[12] = {-2.1f, -1, 0, -0.1f, -1, 0, -0.1f, 1, 0, -2.1f, 1, 0}, quad1[12] = {0.1f, -1, 0, 2.1f, -1, 0, 2.1f, 1, 0, 0.1f, 1, 0};
    const float uv0[8] = {0, 1, 1, 1, 1, 0, 0, 0}, uv1[8] = {0, 2, 2, 2, 2, 0, 0, 0};
    const uint32_t idx[6] = {0, 1, 2, 0, 2, 3};
    brmi_mesh_input meshes[2]{};
    meshes[0].positions = quad0; meshes[1].positions = quad1;
    for (int m = 0; m < 2; m++) { meshes[m].uvs = uv0; meshes[m].vertexCount = 4; meshes[m].indices = idx; meshes[m].indexCount = 6; meshes[m].material = (uint32_t)m; }
    const float* second[2] = {nullptr, uv1};
    brmi_instance_input inst[2]{};
    for (int i = 0; i < 2; i++) { inst[i].mesh = (uint32_t)i; for (int k = 0; k < 4; k++) inst[i].model[k][k] = 1.0f; }
    brmi_view_input view{{0.0f, 0.0f, 3.2f}, 0.0f, 0.0f, 60.0f, 0.1f, 50.0f};
    brmi_scene_params prm{};
    prm.width = 128; prm.height = 72; prm.numPointLights = 1; prm.withDirectionalLight = 1; prm.sizeScale = 1.0f; prm.lodBuilder = BRMI_LOD_BUILDER_OWN;
    brmi_material_inputs in{};
    in.structSize = (uint32_t)sizeof(in);
    in.materials = materials.data(); in.materialCount = (uint32_t)materials.size();
    in.textures = textures.data(); in.textureCount = (uint32_t)textures.size();
    in.samplers = samplers.data(); in.samplerCount = (uint32_t)samplers.size();
    in.uvs1 = second;
    brmi_scene* s = brmi_scene_create_from_meshes_with_materials(&prm, meshes, 2, inst, 2, &view, &in, nullptr, nullptr, nullptr);
    if (!s) { std::printf("null\n"); return 0; }
    HostScene hs;
    take(s, BRMI_ARR_CLOD_MESH_METADATA, hs.meshMetadata); take(s, BRMI_ARR_CLOD_OFFSETS, hs.clodOffsets); take(s, BRMI_ARR_LOD_NODES, hs.lodNodes);
    take(s, BRMI_ARR_LOD_SEGMENTS, hs.lodSegments); take(s, BRMI_ARR_LOD_GROUPS, hs.lodGroups); take(s, BRMI_ARR_GROUP_PAGE_MAP, hs.groupPageMap);
    take(s, BRMI_ARR_PER_MESH, hs.perMesh); take(s, BRMI_ARR_PER_MESH_INSTANCE, hs.perMeshInstance); take(s, BRMI_ARR_MATERIALS, hs.materials);
    take(s, BRMI_ARR_OPENPBR_MATERIALS, hs.openpbrMaterials); take(s, BRMI_ARR_ACTIVE_DRAWS, hs.activeDraws);
    const void* ptr = nullptr; uint64_t bytes = 0; uint32_t count = 0, nTex = 0, nSamp = 0, nSrgb = 0;
    brmi_scene_array(s, BRMI_ARR_PER_OBJECT, &ptr, &bytes, &hs.perObjectCount);
    brmi_scene_array(s, BRMI_ARR_SKINNING_MATRICES, &ptr, &bytes, &hs.skinningMatrixCount);
    brmi_scene_array(s, BRMI_ARR_TEXTURE_DESCS, &ptr, &bytes, &nTex); brmi_scene_array(s, BRMI_ARR_SAMPLER_DESCS, &ptr, &bytes, &nSamp); brmi_scene_array(s, BRMI_ARR_SRGB_TO_LINEAR, &ptr, &bytes, &nSrgb);
    hs.textureTables = !noTables && nTex != 0 && nSamp != 0 && nSrgb != 0;
    count = brmi_scene_slab_count(s);
    hs.slabs.assign(count + 1u, nullptr);
    for (uint32_t i = 1; i <= count; i++) { brmi_scene_slab(s, i, &ptr, &bytes); hs.slabs[i] = static_cast<const uint8_t*>(ptr); }
    // the pages' own word on their UV sets: uvSetCount of the first page's header
    brmi_page_header h0{};
    if (!hs.groupPageMap.empty() && hs.groupPageMap[0].slabDescriptorIndex) std::memcpy(&h0, hs.slabs[hs.groupPageMap[0].slabDescriptorIndex] + hs.groupPageMap[0].slabByteOffset, sizeof(h0));
    const PageHeaderReader reader = [&](uint32_t slab, uint32_t off, uint32_t* n) { std::memcpy(n, hs.slabs[slab] + off, 4); return (int)BRMI_OK; };
    SceneTables t; std::string msg;
    const int rc = analyse_scene(hs, true, 64, true, reader, t, msg);
    std::printf("{\"status\": %d, \"message\": \"%s\", \"hasCoat\": %d, \"hasFuzz\": %d, \"hasAlphaTest\": %d, \"hasTextures\": %d, \"hasParallax\": %d, \"hasVertexColors\": %d, \"uvSets\": %u, "
                "\"pageUvSets\": %u, \"textures\": %u, \"samplers\": %u, \"materials\": %zu, \"totalBits\": %llu}\n", rc, msg.c_str(), t.hasCoat, t.hasFuzz, t.hasAlphaTest, t.hasTextures,
                t.hasParallax, t.hasVertexColors, t.uvSets, h0.uvSetCount, nTex, nSamp, hs.materials.size(), (unsigned long long)t.totalBits);
    brmi_scene_destroy(s);
    return 0;
}
