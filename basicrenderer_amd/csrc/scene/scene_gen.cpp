// scene_gen.cpp -- procedural scenes emitted directly in BasicRenderer's GPU data contract.
//
// Host-only (g++), no GPU code.  Produces, for a preset + seed:
//   * page slabs: 256 KB page tiles, each `header | meshlet descriptors | positions (float3) |
//     oct-snorm16 normals | triangle bytes`, the section order of BuildPackedTriangleMeshPageBlob
//     (BR/src/Mesh/ClusterLODUtilities.cpp:2079-2311);
//   * a cluster-LOD DAG per mesh (groups, segments, group page map) plus one 8-wide BVH per DAG
//     depth hanging off a super-root, with the leaf/internal metric semantics the culling shaders
//     assume (BR/src/Mesh/ClusterLODUtilities.cpp:4606-4900);
//   * per-object / per-mesh / per-instance buffers, camera + culling camera
//     (BR/src/Scene/Scene.cpp:509-535, BR/src/Managers/ViewManager.cpp:19-77), lights
//     (BR/src/Scene/Scene.cpp:222-262), constant-factor materials.
//
// LOD DAGs come from one of three builders (brmi_scene.h, enum brmi_lod_builder): the built-in quadtree (regular-grid decimation of
// parametric patches: level-L meshlets are 8x8-quad tiles sampled at stride 2^L, a group is a 4x4 block of meshlets, the four
// level-(L+1) meshlets that cover a level-L group carry refinedGroup = that group), this library's cluster-LOD builder
// (lod_builder.cpp), or a builder the caller hands in.  This file never loads another library.
#include "brmi_scene.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <fstream>
#include <string>
#include <vector>

namespace {

// ---------------------------------------------------------------------------------------------
struct Pcg32 {
    uint64_t state = 0x853c49e6748fea9bULL, inc = 0xda3e39cb94b95bdbULL;
    explicit Pcg32(uint64_t seed, uint64_t seq = 1) {
        state = 0; inc = (seq << 1u) | 1u; next(); state += seed; next();
    }
    uint32_t next() {
        uint64_t old = state;
        state = old * 6364136223846793005ULL + inc;
        uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u);
        uint32_t rot = (uint32_t)(old >> 59u);
        return (xorshifted >> rot) | (xorshifted << ((32u - rot) & 31u));
    }
    float uniform() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }          // [0,1)
    float range(float a, float b) { return a + (b - a) * uniform(); }
    uint32_t below(uint32_t n) { return n ? next() % n : 0u; }
};

struct V3 { double x, y, z; };
inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 operator*(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double length(V3 a) { return std::sqrt(dot(a, a)); }
inline V3 normalize(V3 a) { double l = length(a); return l > 0 ? a * (1.0 / l) : V3{0, 1, 0}; }

struct Sphere { V3 c; double r; };
Sphere enclose(const std::vector<Sphere>& s) {
    if (s.empty()) return {{0, 0, 0}, 0};
    V3 c{0, 0, 0};
    for (auto& a : s) c = c + a.c;
    c = c * (1.0 / (double)s.size());
    double r = 0;
    for (auto& a : s) r = std::max(r, length(a.c - c) + a.r);
    return {c, r * (1.0 + 1e-5)};
}

struct M4 { double m[4][4]; };
M4 identity() { M4 r{}; for (int i = 0; i < 4; i++) r.m[i][i] = 1; return r; }
M4 mul(const M4& a, const M4& b) {
    M4 r{};
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { double s = 0; for (int k = 0; k < 4; k++) s += a.m[i][k] * b.m[k][j]; r.m[i][j] = s; }
    return r;
}
M4 inverse(const M4& a) {   // Gauss-Jordan in double
    double aug[4][8];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { aug[i][j] = a.m[i][j]; aug[i][j + 4] = (i == j) ? 1.0 : 0.0; }
    for (int col = 0; col < 4; col++) {
        int piv = col;
        for (int r = col + 1; r < 4; r++) if (std::fabs(aug[r][col]) > std::fabs(aug[piv][col])) piv = r;
        if (piv != col) for (int j = 0; j < 8; j++) std::swap(aug[piv][j], aug[col][j]);
        double d = aug[col][col];
        for (int j = 0; j < 8; j++) aug[col][j] /= d;
        for (int r = 0; r < 4; r++) if (r != col) { double f = aug[r][col]; for (int j = 0; j < 8; j++) aug[r][j] -= f * aug[col][j]; }
    }
    M4 r{};
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.m[i][j] = aug[i][j + 4];
    return r;
}
M4 transpose(const M4& a) { M4 r{}; for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) r.m[i][j] = a.m[j][i]; return r; }
void store(float dst[4][4], const M4& a) { for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) dst[i][j] = (float)a.m[i][j]; }
// row-vector convention: p' = p * M ; translation in row 3
M4 translation(V3 t) { M4 r = identity(); r.m[3][0] = t.x; r.m[3][1] = t.y; r.m[3][2] = t.z; return r; }
M4 scaling(double s) { M4 r = identity(); r.m[0][0] = r.m[1][1] = r.m[2][2] = s; return r; }
M4 rotationY(double a) { M4 r = identity(); double c = std::cos(a), s = std::sin(a); r.m[0][0] = c; r.m[0][2] = -s; r.m[2][0] = s; r.m[2][2] = c; return r; }
M4 rotationX(double a) { M4 r = identity(); double c = std::cos(a), s = std::sin(a); r.m[1][1] = c; r.m[1][2] = s; r.m[2][1] = -s; r.m[2][2] = c; return r; }
M4 rotationZ(double a) { M4 r = identity(); double c = std::cos(a), s = std::sin(a); r.m[0][0] = c; r.m[0][1] = s; r.m[1][0] = -s; r.m[1][1] = c; return r; }
V3 xformPoint(V3 p, const M4& m) {
    return {p.x * m.m[0][0] + p.y * m.m[1][0] + p.z * m.m[2][0] + m.m[3][0],
            p.x * m.m[0][1] + p.y * m.m[1][1] + p.z * m.m[2][1] + m.m[3][1],
            p.x * m.m[0][2] + p.y * m.m[1][2] + p.z * m.m[2][2] + m.m[3][2]};
}

// smooth value noise -------------------------------------------------------------------------
inline uint32_t hash3(int x, int y, uint32_t s) {
    uint32_t h = (uint32_t)x * 0x8da6b343u ^ (uint32_t)y * 0xd8163841u ^ s * 0xcb1ab31fu;
    h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15; h *= 0x27d4eb2du; h ^= h >> 13;
    return h;
}
inline double lattice(int x, int y, uint32_t s) { return (double)(hash3(x, y, s) >> 8) * (2.0 / 16777216.0) - 1.0; }
double valueNoise(double x, double y, uint32_t s) {
    double fx = std::floor(x), fy = std::floor(y);
    int ix = (int)fx, iy = (int)fy;
    double tx = x - fx, ty = y - fy;
    tx = tx * tx * (3 - 2 * tx); ty = ty * ty * (3 - 2 * ty);
    double a = lattice(ix, iy, s), b = lattice(ix + 1, iy, s), c = lattice(ix, iy + 1, s), d = lattice(ix + 1, iy + 1, s);
    return (a + (b - a) * tx) + ((c + (d - c) * tx) - (a + (b - a) * tx)) * ty;
}
double fbm(double x, double y, uint32_t s) {
    return 0.6 * valueNoise(x, y, s) + 0.3 * valueNoise(2.03 * x, 2.03 * y, s + 17) + 0.1 * valueNoise(4.1 * x, 4.1 * y, s + 31);
}

// ---------------------------------------------------------------------------------------------
enum PatchType { PATCH_PLANE = 0, PATCH_CYLINDER = 1, PATCH_ELLIPSOID = 2 };
struct PatchDef {
    int type = PATCH_PLANE;
    V3 origin{0, 0, 0}, axisU{1, 0, 0}, axisV{0, 0, 1};   // plane: origin + u*U + v*V ; normal = U x V
    V3 center{0, 0, 0}; double radiusX = 1, radiusY = 1, radiusZ = 1, height = 1;   // cylinder / ellipsoid
    uint32_t nu0 = 1, nv0 = 1;          // meshlets per dimension at LOD 0
    double noiseAmp = 0, noiseFreq = 4; uint32_t noiseSeed = 0;
    double detail = 1;                  // brmi_scene_params::detail: > 1 scales the relief and adds two finer octaves of it
    double reliefSlope = 0;             // brmi_scene_params::reliefSlope: > 0 adds seven octaves whose amplitude is this fraction of their own wavelength
};

// shortest world-space wavelength of the patch's base noise octave, and the world length one unit of the noise displaces
inline void patchNoiseScale(const PatchDef& p, double& wavelength, double& unit) {
    const double f = p.noiseFreq > 0 ? p.noiseFreq : 1.0;
    if (p.type == PATCH_PLANE) { wavelength = std::min(length(p.axisU), length(p.axisV)) / f; unit = 1.0; }
    else if (p.type == PATCH_CYLINDER) { const double r = std::min(p.radiusX, p.radiusZ); wavelength = std::min(2.0 * M_PI * r, p.height) / f; unit = r; }
    else { const double r = std::min(p.radiusX, std::min(p.radiusY, p.radiusZ)); wavelength = M_PI * r / f; unit = r; }
}

V3 evalPatch(const PatchDef& p, double u, double v) {
    double n = p.noiseAmp != 0 ? p.noiseAmp * fbm(u * p.noiseFreq, v * p.noiseFreq, p.noiseSeed) : 0.0;
    if (p.detail > 1.0 && p.noiseAmp != 0) {
        // roughness at every scale: seven more octaves, each half the wavelength and half the amplitude of the one before, so that the
        // simplification error of a LOD level stays proportional to its edge length and the 1-pixel error test keeps pixel-sized triangles
        double a = p.noiseAmp * (p.detail - 1.0) * 0.25, f = p.noiseFreq;
        for (uint32_t k = 1; k <= 7u; k++) { a *= 0.5; f *= 2.0; n += a * valueNoise(u * f, v * f, p.noiseSeed + 101u * k); }
    }
    if (p.reliefSlope > 0.0) {
        // the same roughness at every scale, stated in world units and the same for every patch: octave k (wavelength / 2^k) displaces by
        // reliefSlope x its own wavelength, so a LOD level's simplification error is that fraction of its edge length whatever the patch
        double wl, unit; patchNoiseScale(p, wl, unit);
        double a = p.reliefSlope * wl / unit, f = p.noiseFreq > 0 ? p.noiseFreq : 1.0;
        for (uint32_t k = 1; k <= 7u; k++) { a *= 0.5; f *= 2.0; n += a * valueNoise(u * f, v * f, p.noiseSeed + 101u * k); }
    }
    if (p.type == PATCH_PLANE) {
        V3 nrm = normalize(cross(p.axisU, p.axisV));
        return p.origin + p.axisU * u + p.axisV * v + nrm * n;
    } else if (p.type == PATCH_CYLINDER) {
        // u sweeps the angle so that (dP/du x dP/dv) points outward with v along +Y
        double th = -2.0 * M_PI * u;
        double r = 1.0 + n;
        return {p.center.x + p.radiusX * r * std::cos(th), p.center.y + p.height * v, p.center.z + p.radiusZ * r * std::sin(th)};
    } else {
        double th = -2.0 * M_PI * u;
        double ph = M_PI * (0.04 + 0.92 * v) - 0.5 * M_PI;   // latitude, poles trimmed
        double r = 1.0 + n;
        return {p.center.x + p.radiusX * r * std::cos(ph) * std::cos(th), p.center.y + p.radiusY * r * std::sin(ph),
                p.center.z + p.radiusZ * r * std::cos(ph) * std::sin(th)};
    }
}

struct MeshDef {
    const brmi_mesh_input* user = nullptr;      // the caller's mesh (brmi_scene_create_from_meshes) instead of patches
    const float* userUvs1 = nullptr;            // its second UV set (brmi_material_inputs::uvs1), vertexCount x 2, or null
    std::vector<PatchDef> patches;
    uint32_t lodLevels = 1;      // DAG depth count (1 = flat)
    uint32_t material = 0;
    bool skinned = false;
    double reliefScale = 1.0;    // share of brmi_scene_params::reliefSlope this mesh takes (a street's ground is paved, not a mountain range)
};
struct InstanceDef { uint32_t mesh; M4 model; bool reverseWinding = false; uint32_t skinSlot = 0xFFFFFFFFu; };

uint32_t octEncode(V3 n) {
    n = normalize(n);
    double s = std::fabs(n.x) + std::fabs(n.y) + std::fabs(n.z);
    double ox = n.x / s, oy = n.y / s;
    if (n.z < 0) {
        double tx = (1.0 - std::fabs(oy)) * (ox >= 0 ? 1.0 : -1.0);
        double ty = (1.0 - std::fabs(ox)) * (oy >= 0 ? 1.0 : -1.0);
        ox = tx; oy = ty;
    }
    int qx = (int)std::lround(std::max(-1.0, std::min(1.0, ox)) * 32767.0);
    int qy = (int)std::lround(std::max(-1.0, std::min(1.0, oy)) * 32767.0);
    return ((uint32_t)(uint16_t)(int16_t)qx) | (((uint32_t)(uint16_t)(int16_t)qy) << 16);
}

// per-meshlet build record
struct MeshletBuild {
    uint32_t level, patch, mi, mj, group;
    int32_t  refinedGroup;        // mesh-local, -1 terminal
    std::vector<float> pos;       // 81*3
    std::vector<uint32_t> nrm;    // 81
    std::vector<float> uv;        // V*2 (meshes with a UV set only)
    std::vector<float> uv1;       // V*2: the caller's own second UV set; empty = set k > 0 is derived from set 0 (derivedUv)
    std::vector<uint32_t> color;  // V RGBA8 (materialFeatures bit 5 only)
    std::vector<uint32_t> joints; // V*8 (skinned only)
    std::vector<float> weights;   // V*8
    std::vector<uint8_t> tris;    // 3 local indices per triangle; empty = the implicit 8x8-quad grid over 9x9 vertices
    Sphere bounds;
    uint32_t vertCount() const { return (uint32_t)nrm.size(); }
    uint32_t triCount() const { return tris.empty() ? 128u : (uint32_t)(tris.size() / 3); }
};
struct GroupBuild {
    uint32_t level, patch, gi, gj;
    std::vector<uint32_t> meshlets;    // indices into mesh meshlet list
    Sphere bounds; double error = 0, maxParentError = FLT_MAX; int32_t parent = -1;
    uint32_t firstSegment = 0, segmentCount = 0;
};
struct SegmentBuild { uint32_t group; int32_t refinedGroup; std::vector<uint32_t> meshlets; uint32_t pageIndex = 0, firstMeshletInPage = 0; Sphere cull; };

}  // namespace

struct brmi_scene {
    brmi_scene_params params{};
    std::vector<std::vector<uint8_t>> slabs;       // index 0 unused
    std::vector<brmi_per_object> perObject;
    std::vector<float> normalMatrices;             // 16 floats each
    std::vector<brmi_per_mesh> perMesh;
    std::vector<brmi_per_mesh_instance> perMeshInstance;
    std::vector<brmi_mesh_instance_clod_offsets> clodOffsets;
    std::vector<brmi_clod_mesh_metadata> meshMetadata;
    std::vector<brmi_lod_node> nodes;
    std::vector<brmi_lod_group> groups;
    std::vector<brmi_lod_segment> segments;
    std::vector<brmi_group_page_map_entry> pageMap;
    std::vector<brmi_material_info> materials;
    std::vector<brmi_openpbr_material_info> openpbr;
    std::vector<brmi_light_info> lights;
    std::vector<uint32_t> activeLights;
    std::vector<brmi_camera> cameras;
    std::vector<brmi_culling_camera> cullingCameras;
    std::vector<brmi_view_raster_info> viewRasterInfo;
    std::vector<brmi_per_frame> perFrame;
    std::vector<uint32_t> activeDraws;
    std::vector<float> skinningMatrices;
    std::vector<uint16_t> lutOdE, lutOdAvg, lutImE, lutImAvg; std::vector<float> lutLtc;
    std::vector<brmi_texture_desc> textureDescs;   // texels = byte offset into `texels`
    std::vector<uint8_t> texels;
    std::vector<brmi_sampler_desc> samplerDescs;
    std::vector<float> srgbToLinear;
    uint32_t userUvSets = 0;      // brmi_scene_create_from_meshes_with_materials: UV sets the caller's materials name (0 = the procedural rule)
    brmi_scene_stats stats{};
    std::vector<uint64_t> meshLod0Triangles;        // per mesh: triangles of its finest level
    bool failed = false;                            // a mesh could not be built (the DAG builder failed or returned an inconsistent DAG)
    brmi_dag_build_fn dagBuild = nullptr; brmi_dag_release_fn dagRelease = nullptr; void* dagUser = nullptr;   // lodBuilder EXTERNAL / OWN
    // CLodCache (de)serialisation: what the cache stores per mesh beyond the GPU arrays, and where meshes come from
    struct MeshCacheInfo { uint32_t groupCount = 0, segmentCount = 0, nodeCount = 0, pageCount = 0, maxTraversalDepth = 0;
                           std::vector<float> segmentBounds; std::vector<uint32_t> lodNodeRanges; };   // xyzr per segment; (offset, count) per depth
    std::vector<MeshCacheInfo> meshCache;
    std::string cacheDir;                           // non-empty: buildMesh loads mesh i from <cacheDir>/mesh_<i>.clodbin + .clodmeta
    // page tile allocator
    uint32_t curSlab = 0; uint32_t curSlabPages = 0;
    static constexpr uint32_t kPagesPerSlab = 1024;   // 10-bit page index in the packed cluster
};

namespace {

brmi_group_page_map_entry allocPage(brmi_scene& sc, const std::vector<uint8_t>& blob) {
    if (sc.slabs.empty()) sc.slabs.emplace_back();   // slot 0 = "not resident"
    if (sc.curSlab == 0 || sc.curSlabPages == brmi_scene::kPagesPerSlab) {
        sc.slabs.emplace_back();
        sc.curSlab = (uint32_t)sc.slabs.size() - 1;
        sc.curSlabPages = 0;
    }
    auto& slab = sc.slabs[sc.curSlab];
    uint32_t off = sc.curSlabPages * BRMI_PAGE_SIZE;
    slab.resize((size_t)off + BRMI_PAGE_SIZE, 0);
    std::memcpy(slab.data() + off, blob.data(), blob.size());
    sc.curSlabPages++;
    sc.stats.pages++;
    return {sc.curSlab, off};
}

inline size_t align4(size_t v) { return (v + 3u) & ~size_t(3); }

// Serialise meshlets [list] as one page blob (section order of BuildPackedTriangleMeshPageBlob).
// QuantizeUvOffset / BitsNeededForRange / AppendBits (BR/src/Mesh/ClusterLODUtilities.cpp:58-110,508-517)
uint32_t quantizeUvOffset(float value) {
    const long long scaled = std::llround((double)value * (double)BRMI_UV_QUANTIZATION_SCALE);
    return (uint32_t)std::max(0ll, std::min(scaled, 0xFFFFFFFFll));
}
uint32_t bitsNeededForRange(uint32_t range) { uint32_t b = 0; while (range) { b++; range >>= 1; } return b ? b : 1u; }
void appendBits(std::vector<uint32_t>& words, uint64_t& cursor, uint32_t value, uint32_t bitCount) {
    if (bitCount == 0) return;
    const size_t needWords = (size_t)((cursor + bitCount + 31ull) / 32ull);
    if (words.size() < needWords) words.resize(needWords, 0u);
    const uint64_t off = cursor & 31ull, wi = cursor >> 5, mask = bitCount >= 32u ? 0xFFFFFFFFull : ((1ull << bitCount) - 1ull);
    const uint64_t v = (uint64_t)value & mask;
    words[(size_t)wi] |= (uint32_t)(v << off);
    if (off + bitCount > 32u) words[(size_t)wi + 1] |= (uint32_t)(v >> (32u - off));
    cursor += bitCount;
}

// UV set k > 0 of a vertex: an affine image of set 0 (a different scale, skew and offset per set, so every set has its own gradients and descriptor ranges)
inline void derivedUv(uint32_t set, float u, float v, float& ou, float& ov) {
    if (set == 0u) { ou = u; ov = v; return; }
    const float k = (float)set;
    ou = (0.37f + 0.05f * k) * u + 0.21f * v + 0.11f * k;
    ov = -0.19f * u + (0.43f + 0.03f * k) * v + 0.30f;
}

std::vector<uint8_t> buildPageBlob(const std::vector<const MeshletBuild*>& ms, bool skinned, uint32_t uvSets) {
    const bool hasUv = uvSets != 0u;
    const bool hasColor = !ms.empty() && !ms[0]->color.empty();
    const uint32_t M = (uint32_t)ms.size();
    uint32_t totalVerts = 0, totalTris = 0;
    for (auto* m : ms) { totalVerts += m->vertCount(); totalTris += m->triCount(); }
    brmi_page_header h{};
    h.meshletCount = M;
    h.compressedPositionQuantExp = BRMI_POSITION_FORMAT_FLOAT3;
    h.attributeMask = BRMI_PAGE_ATTRIBUTE_NORMAL | (skinned ? (BRMI_PAGE_ATTRIBUTE_JOINTS | BRMI_PAGE_ATTRIBUTE_WEIGHTS) : 0u) | (hasColor ? BRMI_PAGE_ATTRIBUTE_COLOR : 0u);
    h.uvSetCount = uvSets;
    h.descriptorOffset = (uint32_t)align4(sizeof(brmi_page_header));
    size_t cur = h.descriptorOffset + (size_t)M * sizeof(brmi_meshlet_descriptor);
    h.uvDescriptorOffset = 0;
    // UV sets: descriptors [meshlet][set] (min, 1/65535 scale, bit widths) + one bitstream per set behind a directory (ClusterLODUtilities.cpp:1267-1308,1712-1742)
    std::vector<brmi_meshlet_uv_descriptor> uvDescs((size_t)M * uvSets);
    std::vector<std::vector<uint32_t>> uvWords(uvSets);
    if (hasUv) {
        h.uvDescriptorOffset = (uint32_t)align4(cur);
        cur = h.uvDescriptorOffset + (size_t)M * uvSets * sizeof(brmi_meshlet_uv_descriptor);
        for (uint32_t set = 0; set < uvSets; set++) {
            uint64_t bitCursor = 0;
            for (uint32_t mi = 0; mi < M; mi++) {
                const MeshletBuild* m = ms[mi];
                const uint32_t V = m->vertCount();
                std::vector<float> uv((size_t)V * 2);
                if (set == 1u && m->uv1.size() == (size_t)V * 2) uv = m->uv1;
                else for (uint32_t v = 0; v < V; v++) derivedUv(set, m->uv[v * 2], m->uv[v * 2 + 1], uv[v * 2], uv[v * 2 + 1]);
                float minU = FLT_MAX, minV = FLT_MAX, maxU = -FLT_MAX, maxV = -FLT_MAX;
                for (uint32_t v = 0; v < V; v++) { minU = std::min(minU, uv[v * 2]); maxU = std::max(maxU, uv[v * 2]); minV = std::min(minV, uv[v * 2 + 1]); maxV = std::max(maxV, uv[v * 2 + 1]); }
                if (V == 0) minU = minV = maxU = maxV = 0.0f;
                brmi_meshlet_uv_descriptor d{};
                d.uvBitOffset = (uint32_t)bitCursor;
                d.uvMinU = minU; d.uvMinV = minV; d.uvScaleU = 1.0f / BRMI_UV_QUANTIZATION_SCALE; d.uvScaleV = 1.0f / BRMI_UV_QUANTIZATION_SCALE;
                const uint32_t bitsU = bitsNeededForRange(quantizeUvOffset(std::max(0.0f, maxU - minU))), bitsV = bitsNeededForRange(quantizeUvOffset(std::max(0.0f, maxV - minV)));
                d.uvBits = (bitsU & 0xFFu) | ((bitsV & 0xFFu) << 8);
                const uint32_t maxEncU = bitsU >= 32u ? 0xFFFFFFFFu : ((1u << bitsU) - 1u), maxEncV = bitsV >= 32u ? 0xFFFFFFFFu : ((1u << bitsV) - 1u);
                for (uint32_t v = 0; v < V; v++) {
                    appendBits(uvWords[set], bitCursor, std::min(maxEncU, quantizeUvOffset(std::max(0.0f, uv[v * 2] - minU))), bitsU);
                    appendBits(uvWords[set], bitCursor, std::min(maxEncV, quantizeUvOffset(std::max(0.0f, uv[v * 2 + 1] - minV))), bitsV);
                }
                uvDescs[(size_t)mi * uvSets + set] = d;
            }
        }
    }
    h.positionBitstreamOffset = (uint32_t)align4(cur);
    cur = h.positionBitstreamOffset + (size_t)totalVerts * 12;
    h.normalArrayOffset = (uint32_t)align4(cur);
    cur = h.normalArrayOffset + (size_t)totalVerts * 4;
    h.colorArrayOffset = 0;
    if (hasColor) { h.colorArrayOffset = (uint32_t)align4(cur); cur = h.colorArrayOffset + (size_t)totalVerts * 4; }
    if (skinned) {
        h.jointArrayOffset = (uint32_t)align4(cur); cur = h.jointArrayOffset + (size_t)totalVerts * 32;
        h.weightArrayOffset = (uint32_t)align4(cur); cur = h.weightArrayOffset + (size_t)totalVerts * 32;
    }
    h.uvBitstreamDirectoryOffset = 0;
    std::vector<uint32_t> uvBitstreamOffset(uvSets, 0u);
    if (hasUv) {
        h.uvBitstreamDirectoryOffset = (uint32_t)align4(cur);
        cur = align4(h.uvBitstreamDirectoryOffset + 4u * uvSets);                      // one directory entry per UV set
        for (uint32_t set = 0; set < uvSets; set++) { uvBitstreamOffset[set] = (uint32_t)cur; cur += uvWords[set].size() * 4 + 4; }     // + one word: a 32-bit read may straddle the end
    }
    h.boneIndexStreamOffset = (uint32_t)align4(cur);
    size_t boneWords = 0;
    if (skinned) boneWords = (size_t)M * 4;   // every skinned meshlet lists 4 bones
    cur = h.boneIndexStreamOffset + boneWords * 4;
    h.triangleStreamOffset = (uint32_t)align4(cur);
    cur = h.triangleStreamOffset + (size_t)totalTris * 3;
    std::vector<uint8_t> blob(align4(cur), 0);
    std::memcpy(blob.data(), &h, sizeof(h));
    if (hasUv) {
        std::memcpy(blob.data() + h.uvDescriptorOffset, uvDescs.data(), uvDescs.size() * sizeof(brmi_meshlet_uv_descriptor));
        std::memcpy(blob.data() + h.uvBitstreamDirectoryOffset, uvBitstreamOffset.data(), uvBitstreamOffset.size() * 4);
        for (uint32_t set = 0; set < uvSets; set++) if (!uvWords[set].empty()) std::memcpy(blob.data() + uvBitstreamOffset[set], uvWords[set].data(), uvWords[set].size() * 4);
    }

    uint32_t posCursor = 0, attrCursor = 0, triCursor = 0, boneCursor = 0;
    for (uint32_t i = 0; i < M; i++) {
        const MeshletBuild& m = *ms[i];
        const uint32_t V = (uint32_t)m.nrm.size();
        brmi_meshlet_descriptor d{};
        d.positionBitOffset = posCursor;
        d.vertexAttributeOffset = attrCursor;
        d.triangleByteOffset = triCursor;
        d.boneListOffset = boneCursor;
        d.bitsAndVertexCount = V << 24;
        d.triangleCountAndRefinedGroup = m.triCount() | ((uint32_t)(m.refinedGroup + 1) << 16);
        d.boneCount = skinned ? 4u : 0u;
        d.sourceGroupLocalIndex = m.group;
        d.bounds[0] = (float)m.bounds.c.x; d.bounds[1] = (float)m.bounds.c.y; d.bounds[2] = (float)m.bounds.c.z; d.bounds[3] = (float)m.bounds.r;
        std::memcpy(blob.data() + h.descriptorOffset + (size_t)i * sizeof(d), &d, sizeof(d));
        std::memcpy(blob.data() + h.positionBitstreamOffset + posCursor, m.pos.data(), (size_t)V * 12);
        std::memcpy(blob.data() + h.normalArrayOffset + (size_t)attrCursor * 4, m.nrm.data(), (size_t)V * 4);
        if (hasColor) std::memcpy(blob.data() + h.colorArrayOffset + (size_t)attrCursor * 4, m.color.data(), (size_t)V * 4);
        if (skinned) {
            std::memcpy(blob.data() + h.jointArrayOffset + (size_t)attrCursor * 32, m.joints.data(), (size_t)V * 32);
            std::memcpy(blob.data() + h.weightArrayOffset + (size_t)attrCursor * 32, m.weights.data(), (size_t)V * 32);
            uint32_t bones[4] = {0, 1, 2, 3};
            std::memcpy(blob.data() + h.boneIndexStreamOffset + (size_t)boneCursor * 4, bones, 16);
            boneCursor += 4;
        }
        // 8x8 quads over a 9x9 vertex grid, two CCW triangles per quad (front = +normal side); or the meshlet's own triangle list
        uint8_t* tri = blob.data() + h.triangleStreamOffset + triCursor;
        if (!m.tris.empty()) std::memcpy(tri, m.tris.data(), m.tris.size());
        else for (uint32_t qj = 0; qj < 8; qj++) for (uint32_t qi = 0; qi < 8; qi++) {
            uint8_t a = (uint8_t)(qj * 9 + qi), b = (uint8_t)(a + 1), c = (uint8_t)(a + 10), dd = (uint8_t)(a + 9);
            // alternate the diagonal so neighbouring quads do not all share one direction
            if (((qi + qj) & 1u) == 0) { *tri++ = a; *tri++ = b; *tri++ = c; *tri++ = a; *tri++ = c; *tri++ = dd; }
            else                        { *tri++ = a; *tri++ = b; *tri++ = dd; *tri++ = b; *tri++ = c; *tri++ = dd; }
        }
        posCursor += V * 12; attrCursor += V; triCursor += m.triCount() * 3;
    }
    return blob;
}

size_t meshletPageBytes(const MeshletBuild& m, bool skinned, uint32_t uvSets) {
    return 64 + (size_t)m.vertCount() * 16 + (size_t)m.triCount() * 3 + 4 + (skinned ? (size_t)m.vertCount() * 64 + 16 : 0) + (size_t)uvSets * (32 + (size_t)m.vertCount() * 8 + 8) + (m.color.empty() ? 0 : (size_t)m.vertCount() * 4 + 4);
}

// Built-in LOD DAG: a quadtree over the patch grids (level-L meshlets are 8x8 quads with stride 2^L, groups are 4x4 meshlets).
// PackColorUnorm8 (ClusterLODUtilities.cpp:495-506) of a smooth procedural tint
uint32_t vertexColorOf(double a, double b, uint32_t seed) {
    auto q = [](double x) { return (uint32_t)std::lround(std::max(0.0, std::min(1.0, x)) * 255.0); };
    const double n0 = valueNoise(a * 1.7, b * 1.7, seed ^ 0xC0105u), n1 = valueNoise(a * 2.3 + 5.0, b * 2.3, seed ^ 0xC0106u);
    return q(0.55 + 0.45 * n0) | (q(0.55 + 0.45 * n1) << 8) | (q(0.75 + 0.25 * n0 * n1) << 16) | (0xFFu << 24);
}

uint32_t buildQuadtreeDag(const MeshDef& def, bool hasUv, bool hasColor, std::vector<MeshletBuild>& meshlets, std::vector<GroupBuild>& groups) {
    const uint32_t levels = std::max(1u, std::min(def.lodLevels, 7u));
    // (level, patch) -> first group id and group-grid dims
    struct LevelPatch { uint32_t firstGroup, gw, gh, firstMeshlet, mw, mh; };
    std::vector<std::vector<LevelPatch>> lp(levels, std::vector<LevelPatch>(def.patches.size()));

    for (uint32_t L = 0; L < levels; L++) {
        for (size_t pi = 0; pi < def.patches.size(); pi++) {
            const PatchDef& p = def.patches[pi];
            const uint32_t mw = std::max(1u, p.nu0 >> L), mh = std::max(1u, p.nv0 >> L);
            const uint32_t gw = (mw + 3) / 4, gh = (mh + 3) / 4;
            const uint32_t NU = p.nu0 * 8, NV = p.nv0 * 8;       // LOD0 quads per dim
            const uint32_t su = NU / (mw * 8), sv = NV / (mh * 8); // vertex stride in LOD0 grid units
            lp[L][pi] = {(uint32_t)groups.size(), gw, gh, (uint32_t)meshlets.size(), mw, mh};
            for (uint32_t gj = 0; gj < gh; gj++) for (uint32_t gi = 0; gi < gw; gi++) {
                GroupBuild g{}; g.level = L; g.patch = (uint32_t)pi; g.gi = gi; g.gj = gj; groups.push_back(g);
            }
            for (uint32_t mj = 0; mj < mh; mj++) for (uint32_t mi = 0; mi < mw; mi++) {
                MeshletBuild m{};
                m.level = L; m.patch = (uint32_t)pi; m.mi = mi; m.mj = mj;
                m.refinedGroup = -1;
                if (L > 0) {
                    const LevelPatch& prev = lp[L - 1][pi];
                    uint32_t ci = std::min(2 * mi, prev.mw - 1) / 4, cj = std::min(2 * mj, prev.mh - 1) / 4;
                    m.refinedGroup = (int32_t)(prev.firstGroup + cj * prev.gw + ci);
                }
                m.pos.resize(81 * 3); m.nrm.resize(81);
                if (hasUv) m.uv.resize(81 * 2);
                V3 lo{1e30, 1e30, 1e30}, hi{-1e30, -1e30, -1e30};
                for (uint32_t lj = 0; lj < 9; lj++) for (uint32_t li = 0; li < 9; li++) {
                    double u = (double)((mi * 8 + li) * su) / NU, v = (double)((mj * 8 + lj) * sv) / NV;
                    V3 P = evalPatch(p, u, v);
                    const double hu = 0.25 / NU, hv = 0.25 / NV;
                    V3 du = evalPatch(p, u + hu, v) - evalPatch(p, u - hu, v);
                    V3 dv = evalPatch(p, u, v + hv) - evalPatch(p, u, v - hv);
                    V3 n = cross(du, dv);
                    uint32_t k = lj * 9 + li;
                    m.pos[k * 3 + 0] = (float)P.x; m.pos[k * 3 + 1] = (float)P.y; m.pos[k * 3 + 2] = (float)P.z;
                    m.nrm[k] = octEncode(n);
                    if (hasUv) { m.uv[k * 2] = (float)(u * p.nu0); m.uv[k * 2 + 1] = (float)(v * p.nv0); }   // one texture repeat per LOD-0 meshlet
                    if (hasColor) m.color.push_back(vertexColorOf(u * p.nu0, v * p.nv0, p.noiseSeed));
                    lo = {std::min(lo.x, P.x), std::min(lo.y, P.y), std::min(lo.z, P.z)};
                    hi = {std::max(hi.x, P.x), std::max(hi.y, P.y), std::max(hi.z, P.z)};
                }
                V3 c = (lo + hi) * 0.5; double r = 0;
                for (uint32_t k = 0; k < 81; k++) r = std::max(r, length(V3{m.pos[k * 3], m.pos[k * 3 + 1], m.pos[k * 3 + 2]} - c));
                m.bounds = {c, r * (1.0 + 1e-5) + 1e-7};
                if (def.skinned) {
                    m.joints.assign(81 * 8, 0); m.weights.assign(81 * 8, 0.0f);
                    for (uint32_t k = 0; k < 81; k++) {
                        // 4 influences, weights from the vertex height; bones 0..3 (bounded by the skeleton size)
                        float t = std::min(1.0f, std::max(0.0f, (m.pos[k * 3 + 1] - (float)lo.y) / (float)std::max(1e-6, hi.y - lo.y)));
                        float w[4] = {(1 - t) * (1 - t), 2 * t * (1 - t) * 0.5f, 2 * t * (1 - t) * 0.5f, t * t};
                        for (int q = 0; q < 4; q++) { m.joints[k * 8 + q] = (uint32_t)q; m.weights[k * 8 + q] = w[q]; }
                    }
                }
                uint32_t gid = lp[L][pi].firstGroup + (mj / 4) * gw + (mi / 4);
                m.group = gid;
                groups[gid].meshlets.push_back((uint32_t)meshlets.size());
                meshlets.push_back(std::move(m));
            }
        }
    }
    // group bounds (nested) and errors (monotone)
    for (uint32_t L = 0; L < levels; L++) {
        for (size_t pi = 0; pi < def.patches.size(); pi++) {
            const LevelPatch& cur = lp[L][pi];
            const PatchDef& p = def.patches[pi];
            for (uint32_t gj = 0; gj < cur.gh; gj++) for (uint32_t gi = 0; gi < cur.gw; gi++) {
                GroupBuild& g = groups[cur.firstGroup + gj * cur.gw + gi];
                std::vector<Sphere> parts;
                double childErr = 0;
                if (L == 0) {
                    for (uint32_t mi : g.meshlets) parts.push_back(meshlets[mi].bounds);
                } else {
                    // children = level L-1 groups referenced by this group's meshlets
                    std::vector<int32_t> kids;
                    for (uint32_t mi : g.meshlets) kids.push_back(meshlets[mi].refinedGroup);
                    std::sort(kids.begin(), kids.end()); kids.erase(std::unique(kids.begin(), kids.end()), kids.end());
                    for (int32_t k : kids) { parts.push_back(groups[k].bounds); childErr = std::max(childErr, groups[k].error); groups[k].parent = (int32_t)(&g - groups.data()); }
                    for (uint32_t mi : g.meshlets) parts.push_back(meshlets[mi].bounds);
                }
                g.bounds = enclose(parts);
                // own representation error: deviation of dropped level-(L-1) vertices from level-L edges
                double dev = 0;
                if (L > 0) {
                    const uint32_t NU = p.nu0 * 8, NV = p.nv0 * 8;
                    const uint32_t su = NU / (cur.mw * 8), sv = NV / (cur.mh * 8);
                    for (uint32_t mi : g.meshlets) {
                        const MeshletBuild& m = meshlets[mi];
                        for (uint32_t lj = 0; lj < 8; lj++) for (uint32_t li = 0; li < 8; li++) {
                            // midpoint of the quad vs. true surface
                            double u = ((m.mi * 8 + li) * su + 0.5 * su) / NU, v = ((m.mj * 8 + lj) * sv + 0.5 * sv) / NV;
                            V3 P = evalPatch(p, u, v);
                            auto at = [&](uint32_t a, uint32_t b) { uint32_t k = b * 9 + a; return V3{m.pos[k * 3], m.pos[k * 3 + 1], m.pos[k * 3 + 2]}; };
                            V3 Q = (at(li, lj) + at(li + 1, lj) + at(li, lj + 1) + at(li + 1, lj + 1)) * 0.25;
                            dev = std::max(dev, length(P - Q));
                        }
                    }
                }
                g.error = (L == 0) ? 0.0 : std::max(childErr * 1.0001 + 1e-9, childErr + dev);
            }
        }
    }
    for (auto& g : groups) g.maxParentError = (g.parent >= 0) ? groups[g.parent].error : (double)FLT_MAX;
    return levels;
}

// LOD DAG from a cluster-LOD builder (lod_builder.cpp, or the caller's): the patches are tessellated at their LOD0 resolution into one
// indexed mesh, the builder clusters / groups / simplifies it, and its output (a brmi_dag) is mapped onto the build records:
//   group  -> LOD group: bounds and error of `clodGroup::simplified` (the test "is this group's simplification too coarse", rule 1,
//             and through `refined` rule 2 of clusterlod.h)
//   cluster -> meshlet with its own vertex / triangle counts, `refined` = refinedGroup
// Returns the number of DAG depths, 0 on failure.
uint32_t buildClusterLodDag(const brmi_scene& sc, const MeshDef& def, bool hasUv, bool hasColor, std::vector<MeshletBuild>& meshlets, std::vector<GroupBuild>& groups) {
    if (!sc.dagBuild) return 0;
    std::vector<float> pos, nrm, uvs; std::vector<uint32_t> idx, colors;
    if (def.user) {
        const brmi_mesh_input& u = *def.user;
        const size_t V = u.vertexCount;
        pos.assign(u.positions, u.positions + V * 3); idx.assign(u.indices, u.indices + u.indexCount);
        if (u.normals) nrm.assign(u.normals, u.normals + V * 3);
        else {      // area-weighted vertex normals
            std::vector<V3> acc(V, V3{0, 0, 0});
            for (size_t t = 0; t + 2 < idx.size(); t += 3) {
                const uint32_t a = idx[t], b = idx[t + 1], c = idx[t + 2];
                const V3 pa{pos[a * 3], pos[a * 3 + 1], pos[a * 3 + 2]}, pb{pos[b * 3], pos[b * 3 + 1], pos[b * 3 + 2]}, pc{pos[c * 3], pos[c * 3 + 1], pos[c * 3 + 2]};
                const V3 n = cross(pb - pa, pc - pa);
                acc[a] = acc[a] + n; acc[b] = acc[b] + n; acc[c] = acc[c] + n;
            }
            nrm.resize(V * 3);
            for (size_t v = 0; v < V; v++) {
                const double l = std::sqrt(dot(acc[v], acc[v]));
                const V3 n = l > 0 ? acc[v] * (1.0 / l) : V3{0, 1, 0};
                nrm[v * 3] = (float)n.x; nrm[v * 3 + 1] = (float)n.y; nrm[v * 3 + 2] = (float)n.z;
            }
        }
        if (u.uvs) uvs.assign(u.uvs, u.uvs + V * 2); else uvs.assign(V * 2, 0.0f);
        if (u.colors) colors.assign(u.colors, u.colors + V); else colors.assign(V, 0xFFFFFFFFu);
    }
    for (const PatchDef& p : def.patches) {
        const uint32_t NU = p.nu0 * 8, NV = p.nv0 * 8, base = (uint32_t)(pos.size() / 3);
        for (uint32_t j = 0; j <= NV; j++) for (uint32_t i = 0; i <= NU; i++) {
            const double u = (double)i / NU, v = (double)j / NV;
            const V3 P = evalPatch(p, u, v);
            const double hu = 0.25 / NU, hv = 0.25 / NV;
            const V3 n = normalize(cross(evalPatch(p, u + hu, v) - evalPatch(p, u - hu, v), evalPatch(p, u, v + hv) - evalPatch(p, u, v - hv)));
            pos.push_back((float)P.x); pos.push_back((float)P.y); pos.push_back((float)P.z);
            nrm.push_back((float)n.x); nrm.push_back((float)n.y); nrm.push_back((float)n.z);
            uvs.push_back((float)(u * p.nu0)); uvs.push_back((float)(v * p.nv0));
            colors.push_back(vertexColorOf(u * p.nu0, v * p.nv0, p.noiseSeed));
        }
        for (uint32_t qj = 0; qj < NV; qj++) for (uint32_t qi = 0; qi < NU; qi++) {
            const uint32_t a = base + qj * (NU + 1) + qi, b = a + 1, c = a + NU + 2, d = a + NU + 1;
            if (((qi + qj) & 1u) == 0) { idx.insert(idx.end(), {a, b, c, a, c, d}); } else { idx.insert(idx.end(), {a, b, d, b, c, d}); }
        }
    }
    brmi_dag dag{};
    if (sc.dagBuild(sc.dagUser, pos.data(), pos.size() / 3, idx.data(), idx.size(), nrm.data(), &dag) != 0) return 0;
    struct Release { const brmi_scene& sc; brmi_dag& d; ~Release() { if (sc.dagRelease) sc.dagRelease(sc.dagUser, &d); } } release{sc, dag};
    const uint32_t nG = dag.groupCount, nC = dag.clusterCount;
    const brmi_dag_group* g = dag.groups; const brmi_dag_cluster* c = dag.clusters; const uint32_t* vref = dag.vertexRefs; const uint8_t* tri = dag.triangles;
    // the kernels index what follows unchecked: refuse a DAG whose cross references or limits are off
    if (nG == 0 || nC == 0 || !g || !c || !vref || !tri) return 0;
    for (uint32_t ci = 0; ci < nC; ci++) {
        const brmi_dag_cluster& k = c[ci];
        if (k.group < 0 || (uint32_t)k.group >= nG || k.refined >= (int32_t)nG || k.vertexCount == 0 || k.vertexCount > BRMI_MESHLET_MAX_VERTS || k.triangleCount == 0 || k.triangleCount > BRMI_MESHLET_MAX_TRIS ||
            (uint64_t)k.firstVertex + k.vertexCount > dag.vertexRefCount || (uint64_t)k.firstTriangleByte + (uint64_t)k.triangleCount * 3u > dag.triangleBytes) return 0;
        for (uint32_t v = 0; v < k.vertexCount; v++) if (vref[k.firstVertex + v] >= pos.size() / 3) return 0;
        for (uint32_t t = 0; t < k.triangleCount * 3u; t++) if (tri[k.firstTriangleByte + t] >= k.vertexCount) return 0;
    }
    uint32_t levels = 1;
    groups.resize(nG);
    for (uint32_t gi = 0; gi < nG; gi++) {
        GroupBuild& o = groups[gi];
        o.level = (uint32_t)std::max(0, g[gi].depth); o.patch = 0; o.gi = gi; o.gj = 0;
        o.bounds = {V3{g[gi].center[0], g[gi].center[1], g[gi].center[2]}, (double)g[gi].radius};
        o.maxParentError = g[gi].error >= FLT_MAX ? (double)FLT_MAX : (double)g[gi].error;
        o.error = 0; o.parent = -1;
        levels = std::max(levels, o.level + 1);
    }
    meshlets.reserve(nC);
    for (uint32_t ci = 0; ci < nC; ci++) {
        const brmi_dag_cluster& k = c[ci];
        MeshletBuild m{};
        m.level = groups[k.group].level; m.patch = 0; m.mi = ci; m.mj = 0; m.group = (uint32_t)k.group; m.refinedGroup = k.refined;
        const uint32_t V = k.vertexCount, T = k.triangleCount;
        m.pos.resize((size_t)V * 3); m.nrm.resize(V);
        if (hasUv) m.uv.resize((size_t)V * 2);
        V3 lo{1e30, 1e30, 1e30}, hi{-1e30, -1e30, -1e30};
        for (uint32_t v = 0; v < V; v++) {
            const uint32_t src = vref[k.firstVertex + v];
            if (hasUv) { m.uv[(size_t)v * 2] = uvs[(size_t)src * 2]; m.uv[(size_t)v * 2 + 1] = uvs[(size_t)src * 2 + 1]; }
            if (hasUv && def.user && def.userUvs1) { m.uv1.push_back(def.userUvs1[(size_t)src * 2]); m.uv1.push_back(def.userUvs1[(size_t)src * 2 + 1]); }
            if (hasColor) m.color.push_back(colors[src]);
            for (int q = 0; q < 3; q++) m.pos[v * 3 + q] = pos[(size_t)src * 3 + q];
            m.nrm[v] = octEncode(V3{nrm[(size_t)src * 3], nrm[(size_t)src * 3 + 1], nrm[(size_t)src * 3 + 2]});
            lo = {std::min(lo.x, (double)m.pos[v * 3]), std::min(lo.y, (double)m.pos[v * 3 + 1]), std::min(lo.z, (double)m.pos[v * 3 + 2])};
            hi = {std::max(hi.x, (double)m.pos[v * 3]), std::max(hi.y, (double)m.pos[v * 3 + 1]), std::max(hi.z, (double)m.pos[v * 3 + 2])};
        }
        m.tris.assign(tri + k.firstTriangleByte, tri + k.firstTriangleByte + (size_t)T * 3);
        // the builder's sphere (optimize_bounds), widened if float rounding left a vertex outside
        const V3 cc{k.center[0], k.center[1], k.center[2]};
        double r = k.radius;
        for (uint32_t v = 0; v < V; v++) r = std::max(r, length(V3{m.pos[v * 3], m.pos[v * 3 + 1], m.pos[v * 3 + 2]} - cc));
        m.bounds = {cc, r * (1.0 + 1e-5) + 1e-7};
        if (def.skinned) {
            m.joints.assign((size_t)V * 8, 0); m.weights.assign((size_t)V * 8, 0.0f);
            for (uint32_t v = 0; v < V; v++) {
                float t = std::min(1.0f, std::max(0.0f, (m.pos[v * 3 + 1] - (float)lo.y) / (float)std::max(1e-6, hi.y - lo.y)));
                float w[4] = {(1 - t) * (1 - t), 2 * t * (1 - t) * 0.5f, 2 * t * (1 - t) * 0.5f, t * t};
                for (int q = 0; q < 4; q++) { m.joints[(size_t)v * 8 + q] = (uint32_t)q; m.weights[(size_t)v * 8 + q] = w[q]; }
            }
        }
        groups[k.group].meshlets.push_back((uint32_t)meshlets.size());
        groups[k.group].error = std::max(groups[k.group].error, (double)k.error);
        if (k.refined >= 0 && groups[k.refined].parent < 0) groups[k.refined].parent = k.group;
        meshlets.push_back(std::move(m));
    }
    return levels;
}

// Build one mesh: LOD DAG (built-in quadtree or the reference's builder), then segments, pages, groups and the 8-wide BVH.
bool loadCachedMesh(brmi_scene& sc, const MeshDef& def, uint32_t meshIndex);

bool buildMesh(brmi_scene& sc, const MeshDef& defIn, uint32_t meshIndex) {
    MeshDef def = defIn;
    for (PatchDef& pd : def.patches) { pd.detail = sc.params.detail; pd.reliefSlope = sc.params.reliefSlope > 0.0f ? sc.params.reliefSlope * def.reliefScale : 0.0; }
    if (!sc.cacheDir.empty()) { if (!loadCachedMesh(sc, def, meshIndex)) { sc.failed = true; return false; } return true; }
    std::vector<MeshletBuild> meshlets;
    std::vector<GroupBuild> groups;
    const bool hasUv = (sc.params.materialFeatures & 24u) != 0u, hasColor = (sc.params.materialFeatures & 32u) != 0u;
    const uint32_t uvSets = hasUv ? (sc.userUvSets ? sc.userUvSets : ((sc.params.materialFeatures & 256u) ? 3u : 1u)) : 0u;       // materialFeatures bit 8: pages carry three UV sets; the caller's materials: the sets they name
    const uint32_t levels = sc.params.lodBuilder != BRMI_LOD_BUILDER_QUADTREE ? buildClusterLodDag(sc, def, hasUv, hasColor, meshlets, groups) : buildQuadtreeDag(def, hasUv, hasColor, meshlets, groups);
    if (levels == 0) { sc.failed = true; return false; }

    // segments: partition each group's meshlets by refinedGroup (stable)
    std::vector<SegmentBuild> segs;
    for (size_t gi = 0; gi < groups.size(); gi++) {
        GroupBuild& g = groups[gi];
        g.firstSegment = (uint32_t)segs.size();
        std::vector<int32_t> keys;
        for (uint32_t mi : g.meshlets) if (std::find(keys.begin(), keys.end(), meshlets[mi].refinedGroup) == keys.end()) keys.push_back(meshlets[mi].refinedGroup);
        for (int32_t k : keys) {
            // one segment per (group, refined group); a segment that would not fit a 256 KB page is cut into several
            SegmentBuild s{}; s.group = (uint32_t)gi; s.refinedGroup = k;
            std::vector<Sphere> parts; size_t bytes = 0;
            auto close = [&]() { if (s.meshlets.empty()) return; s.cull = enclose(parts); segs.push_back(s); s.meshlets.clear(); parts.clear(); bytes = 0; };
            for (uint32_t mi : g.meshlets) if (meshlets[mi].refinedGroup == k) {
                const size_t need = meshletPageBytes(meshlets[mi], def.skinned, uvSets);
                if (bytes + need + 256 > BRMI_PAGE_SIZE) close();
                s.meshlets.push_back(mi); parts.push_back(meshlets[mi].bounds); bytes += need;
            }
            close();
        }
        g.segmentCount = (uint32_t)segs.size() - g.firstSegment;
    }

    // pages: pack segments sequentially
    const uint32_t pageMapBase = (uint32_t)sc.pageMap.size();
    {
        std::vector<const MeshletBuild*> cur;
        std::vector<size_t> curSegs;
        size_t bytes = 64;
        auto flush = [&]() {
            if (cur.empty()) return;
            auto blob = buildPageBlob(cur, def.skinned, uvSets);
            sc.pageMap.push_back(allocPage(sc, blob));
            cur.clear(); curSegs.clear(); bytes = 64;
        };
        for (size_t si = 0; si < segs.size(); si++) {
            size_t need = 64; for (uint32_t mi : segs[si].meshlets) need += meshletPageBytes(meshlets[mi], def.skinned, uvSets);
            if (bytes + need > BRMI_PAGE_SIZE) flush();
            segs[si].pageIndex = (uint32_t)(sc.pageMap.size() - pageMapBase);
            segs[si].firstMeshletInPage = (uint32_t)cur.size();
            for (uint32_t mi : segs[si].meshlets) cur.push_back(&meshlets[mi]);
            bytes += need;
        }
        flush();
    }

    // emit groups / segments
    const uint32_t groupsBase = (uint32_t)sc.groups.size(), segmentsBase = (uint32_t)sc.segments.size();
    uint32_t runningMeshlet = 0;
    for (auto& g : groups) {
        brmi_lod_group o{};
        o.centerAndRadius[0] = (float)g.bounds.c.x; o.centerAndRadius[1] = (float)g.bounds.c.y; o.centerAndRadius[2] = (float)g.bounds.c.z; o.centerAndRadius[3] = (float)g.bounds.r;
        o.error = (float)g.error;
        o.firstMeshlet = runningMeshlet; o.meshletCount = (uint32_t)g.meshlets.size(); runningMeshlet += o.meshletCount;
        o.depth = (int32_t)g.level;
        o.firstSegment = g.firstSegment; o.segmentCount = g.segmentCount;
        o.terminalSegmentCount = (g.level == 0) ? g.segmentCount : 0;
        o.flags = 0; o.pageMapBase = 0; o.pageCount = 0;
        o.parentGroupId = g.parent;
        o.maxParentError = g.maxParentError >= (double)FLT_MAX ? FLT_MAX : (float)g.maxParentError;
        o.representationError = (float)g.error;
        sc.groups.push_back(o);
    }
    for (auto& s : segs) sc.segments.push_back({s.refinedGroup, s.firstMeshletInPage, (uint32_t)s.meshlets.size(), s.pageIndex});
    brmi_scene::MeshCacheInfo ci;
    ci.groupCount = (uint32_t)groups.size(); ci.segmentCount = (uint32_t)segs.size(); ci.pageCount = (uint32_t)sc.pageMap.size() - pageMapBase;
    for (auto& sg : segs) { ci.segmentBounds.push_back((float)sg.cull.c.x); ci.segmentBounds.push_back((float)sg.cull.c.y); ci.segmentBounds.push_back((float)sg.cull.c.z); ci.segmentBounds.push_back((float)sg.cull.r); }

    // BVH: node 0 super-root, nodes 1..levels depth roots, then per-depth subtrees
    struct BNode { brmi_lod_node n; std::vector<uint32_t> kids; Sphere cull, lod; double err; };
    std::vector<BNode> bn(1 + levels);
    uint32_t maxTreeDepth = 1;
    auto setMetric = [](BNode& b) {
        b.n.cullCenterAndRadius[0] = (float)b.cull.c.x; b.n.cullCenterAndRadius[1] = (float)b.cull.c.y; b.n.cullCenterAndRadius[2] = (float)b.cull.c.z; b.n.cullCenterAndRadius[3] = (float)b.cull.r;
        b.n.lodCenterAndRadius[0] = (float)b.lod.c.x; b.n.lodCenterAndRadius[1] = (float)b.lod.c.y; b.n.lodCenterAndRadius[2] = (float)b.lod.c.z; b.n.lodCenterAndRadius[3] = (float)b.lod.r;
        b.n.maxQuadricError = b.err >= (double)FLT_MAX ? FLT_MAX : (float)b.err;
    };
    for (uint32_t L = 0; L < levels; L++) {
        ci.lodNodeRanges.push_back((uint32_t)bn.size());      // nodes of depth L (besides its root at slot 1 + L) start here
        // leaves of this depth
        std::vector<BNode> level;
        for (size_t si = 0; si < segs.size(); si++) {
            const GroupBuild& g = groups[segs[si].group];
            if (g.level != L) continue;
            BNode b{}; b.n.isLeaf = BRMI_NODE_SEGMENT_LEAF; b.n.indexOrOffset = (uint32_t)si;
            b.n.countMinusOne = (uint32_t)(segs[si].refinedGroup + 1); b.n.ownerGroupId = segs[si].group;
            std::vector<Sphere> both{segs[si].cull};
            b.cull = enclose(both); b.lod = g.bounds; b.err = g.maxParentError;
            level.push_back(std::move(b));
        }
        // spatial order: Morton code of the cull centre inside the depth's bbox
        V3 lo{1e30, 1e30, 1e30}, hi{-1e30, -1e30, -1e30};
        for (auto& b : level) { lo = {std::min(lo.x, b.cull.c.x), std::min(lo.y, b.cull.c.y), std::min(lo.z, b.cull.c.z)}; hi = {std::max(hi.x, b.cull.c.x), std::max(hi.y, b.cull.c.y), std::max(hi.z, b.cull.c.z)}; }
        auto morton = [&](const BNode& b) {
            auto q = [](double v, double a, double c) { double t = c > a ? (v - a) / (c - a) : 0.0; return (uint32_t)std::min(1023.0, std::max(0.0, t * 1023.0)); };
            auto spread = [](uint32_t v) { v &= 0x3FF; v = (v | (v << 16)) & 0x30000FF; v = (v | (v << 8)) & 0x300F00F; v = (v | (v << 4)) & 0x30C30C3; v = (v | (v << 2)) & 0x9249249; return v; };
            return spread(q(b.cull.c.x, lo.x, hi.x)) | (spread(q(b.cull.c.y, lo.y, hi.y)) << 1) | (spread(q(b.cull.c.z, lo.z, hi.z)) << 2);
        };
        std::stable_sort(level.begin(), level.end(), [&](const BNode& a, const BNode& b) { return morton(a) < morton(b); });
        // bottom-up: collapse 8 at a time; keep every tier so we can lay children out contiguously
        std::vector<std::vector<BNode>> tiers; tiers.push_back(std::move(level));
        while (tiers.back().size() > 1) {
            auto& below = tiers.back();
            std::vector<BNode> up;
            for (size_t i = 0; i < below.size(); i += 8) {
                BNode b{}; b.n.isLeaf = BRMI_NODE_INTERNAL;
                std::vector<Sphere> cs, ls; double e = 0;
                for (size_t k = i; k < std::min(below.size(), i + 8); k++) { b.kids.push_back((uint32_t)k); cs.push_back(below[k].cull); ls.push_back(below[k].lod); e = std::max(e, below[k].err); }
                b.cull = enclose(cs); b.lod = enclose(ls); b.err = e;
                up.push_back(std::move(b));
            }
            tiers.push_back(std::move(up));
        }
        maxTreeDepth = std::max(maxTreeDepth, (uint32_t)tiers.size() + 1);
        struct Finish { std::vector<uint32_t>& r; std::vector<BNode>& b; ~Finish() { r.push_back((uint32_t)b.size() - r.back()); } } finish{ci.lodNodeRanges, bn};
        // lay out top-down; tier T-1 is the depth root -> global slot 1+L
        std::vector<std::vector<uint32_t>> slot(tiers.size());
        for (size_t t = 0; t < tiers.size(); t++) slot[t].assign(tiers[t].size(), 0);
        slot[tiers.size() - 1][0] = 1 + L;
        for (size_t t = tiers.size(); t-- > 0;) {
            for (size_t i = 0; i < tiers[t].size(); i++) {
                BNode& b = tiers[t][i];
                if (b.n.isLeaf == BRMI_NODE_INTERNAL) {
                    uint32_t first = (uint32_t)bn.size();
                    for (size_t k = 0; k < b.kids.size(); k++) { slot[t - 1][b.kids[k]] = first + (uint32_t)k; bn.emplace_back(); }
                    b.n.indexOrOffset = first; b.n.countMinusOne = (uint32_t)b.kids.size() - 1; b.n.ownerGroupId = 0;
                }
                setMetric(b);
                bn[slot[t][i]] = b;
            }
        }
    }
    {   // super-root
        BNode& r = bn[0]; r.n.isLeaf = BRMI_NODE_INTERNAL; r.n.indexOrOffset = 1; r.n.countMinusOne = levels - 1;
        std::vector<Sphere> cs, ls; for (uint32_t L = 0; L < levels; L++) { cs.push_back(bn[1 + L].cull); ls.push_back(bn[1 + L].lod); }
        r.cull = enclose(cs); r.lod = enclose(ls); r.err = (double)FLT_MAX; setMetric(r);
    }
    const uint32_t nodesBase = (uint32_t)sc.nodes.size();
    for (auto& b : bn) sc.nodes.push_back(b.n);
    ci.nodeCount = (uint32_t)bn.size(); ci.maxTraversalDepth = maxTreeDepth;
    sc.meshCache.push_back(std::move(ci));

    brmi_clod_mesh_metadata md{};
    md.groupsBase = groupsBase; md.segmentsBase = segmentsBase; md.lodNodesBase = nodesBase; md.rootNode = 0;
    md.pageMapBase = pageMapBase; md.lodLevelCount = levels; md.maxDepth = maxTreeDepth;
    sc.meshMetadata.push_back(md);

    brmi_per_mesh pm{};
    pm.materialDataIndex = def.material; pm.rasterBucketIndex = 0;
    pm.vertexFlags = (1u << 1) | (def.skinned ? BRMI_VERTEX_SKINNED : 0u) | (hasColor ? 1u : 0u) | (hasUv ? (1u << 2) : 0u);
    pm.vertexByteSize = 24;
    pm.boundingSphere[0] = bn[0].n.cullCenterAndRadius[0]; pm.boundingSphere[1] = bn[0].n.cullCenterAndRadius[1];
    pm.boundingSphere[2] = bn[0].n.cullCenterAndRadius[2]; pm.boundingSphere[3] = bn[0].n.cullCenterAndRadius[3];
    uint32_t lod0 = 0, lod0Verts = 0; uint64_t lod0Tris = 0;
    for (auto& m : meshlets) if (m.level == 0) { lod0++; lod0Verts += m.vertCount(); lod0Tris += m.triCount(); }
    pm.clodNumMeshlets = (uint32_t)meshlets.size(); pm.numMeshlets = lod0; pm.numVertices = lod0Verts;
    sc.perMesh.push_back(pm);
    sc.meshLod0Triangles.push_back(lod0Tris);

    sc.stats.meshletsTotal += (uint32_t)meshlets.size(); sc.stats.meshletsLod0 += lod0;
    sc.stats.uniqueTriangles += lod0Tris;
    sc.stats.maxBvhDepth = std::max(sc.stats.maxBvhDepth, maxTreeDepth);
    sc.stats.lodLevelsMax = std::max(sc.stats.lodLevelsMax, levels);
    (void)meshIndex;
    return true;
}

// ---- CLodCache: the reference's on-disk form of one mesh's cluster-LOD data ----------------------------------------------------
// container  "<name>.clodbin": ContainerHeader {magic 'CLOD', version 4, reserved, pageCount}, a directory of pageCount
//            ClusterLODGroupDiskLocator {u64 blobOffset, u32 blobSizeBytes, u32 reserved}, then the page blobs
//            (SaveContainerPayload / OpenContainerFile, BR/src/Import/CLodCache.cpp:252-259,309-374,1000-1020);
// metadata   the byte blob of SerializeMetadata (CLodCache.cpp:171-211), schema 47: POD vectors are u64 count + elements, strings
//            u64 length + bytes.  The reference stores this blob as the `clodBlob` uchar-array attribute of a USD crate file
//            (CLodCache.cpp:528-560), which needs OpenUSD to open; here the blob is a plain file ("<name>.clodmeta").
constexpr uint32_t kClodContainerMagic = 0x444F4C43u, kClodContainerVersion = 4u, kClodSchemaVersion = 47u;
struct ClodDiskLocator { uint64_t blobOffset; uint32_t blobSizeBytes, reserved; };
struct ClodNodeRange { uint32_t offset, count; };

struct MeshCacheData {
    std::vector<brmi_lod_group> groups; std::vector<brmi_lod_segment> segments; std::vector<float> segmentBounds; float objectSphere[4] = {0, 0, 0, 0};
    std::vector<uint32_t> groupPageReferences, groupPageReferenceOffsets;
    uint32_t trianglePageCount = 0;
    std::vector<brmi_lod_node> nodes; std::vector<ClodNodeRange> lodNodeRanges; std::vector<uint32_t> lodLevelRoots;
    uint32_t maxDepth = 0, maxTraversalDepth = 0;
    std::vector<std::vector<uint8_t>> pages;
    uint64_t buildConfigHash = 0; std::string sourceIdentifier, primPath, subsetName, containerFileName;
};

template <typename T> void putPod(std::vector<uint8_t>& o, const T& v) { const uint8_t* p = reinterpret_cast<const uint8_t*>(&v); o.insert(o.end(), p, p + sizeof(T)); }
template <typename T> void putVec(std::vector<uint8_t>& o, const std::vector<T>& v) { putPod(o, (uint64_t)v.size()); if (!v.empty()) { const uint8_t* p = reinterpret_cast<const uint8_t*>(v.data()); o.insert(o.end(), p, p + sizeof(T) * v.size()); } }
void putStr(std::vector<uint8_t>& o, const std::string& v) { putPod(o, (uint64_t)v.size()); o.insert(o.end(), v.begin(), v.end()); }
template <typename T> bool getPod(const std::vector<uint8_t>& in, size_t& off, T& v) { if (off + sizeof(T) > in.size()) return false; std::memcpy(&v, in.data() + off, sizeof(T)); off += sizeof(T); return true; }
template <typename T> bool getVec(const std::vector<uint8_t>& in, size_t& off, std::vector<T>& v) {
    uint64_t n = 0; if (!getPod(in, off, n)) return false;
    if (n > (in.size() - off) / sizeof(T)) return false;
    v.resize((size_t)n); if (n) std::memcpy(v.data(), in.data() + off, sizeof(T) * (size_t)n); off += sizeof(T) * (size_t)n; return true;
}
bool getStr(const std::vector<uint8_t>& in, size_t& off, std::string& v) { uint64_t n = 0; if (!getPod(in, off, n) || n > in.size() - off) return false; v.assign(reinterpret_cast<const char*>(in.data() + off), (size_t)n); off += (size_t)n; return true; }

std::vector<uint8_t> serializeClodMetadata(const MeshCacheData& d, const std::vector<ClodDiskLocator>& pageLocators) {
    std::vector<uint8_t> o;
    putPod(o, kClodSchemaVersion); putPod(o, d.buildConfigHash);
    putVec(o, d.groups); putVec(o, d.segments);
    putPod(o, (uint64_t)(d.segmentBounds.size() / 4)); { const uint8_t* p = reinterpret_cast<const uint8_t*>(d.segmentBounds.data()); o.insert(o.end(), p, p + d.segmentBounds.size() * 4); }
    o.insert(o.end(), reinterpret_cast<const uint8_t*>(d.objectSphere), reinterpret_cast<const uint8_t*>(d.objectSphere) + 16);
    putPod(o, (uint8_t)0);                                            // no inline group chunks
    putVec(o, std::vector<ClodDiskLocator>{});                        // groupDiskLocators (per-group files: the pre-container layout)
    putVec(o, pageLocators);
    putVec(o, d.groupPageReferences); putVec(o, d.groupPageReferenceOffsets);
    putPod(o, d.trianglePageCount); putPod(o, d.trianglePageCount /* voxelPageBase */); putPod(o, (uint32_t)0 /* voxelPageCount */);
    putStr(o, d.sourceIdentifier); putStr(o, d.primPath); putStr(o, d.subsetName); putPod(o, d.buildConfigHash); putStr(o, d.containerFileName);
    putVec(o, d.nodes); putVec(o, d.lodNodeRanges); putVec(o, d.lodLevelRoots);
    putPod(o, d.maxDepth); putPod(o, d.maxTraversalDepth);
    return o;
}
bool deserializeClodMetadata(const std::vector<uint8_t>& in, MeshCacheData& d, std::vector<ClodDiskLocator>& pageLocators) {
    size_t off = 0; uint32_t schema = 0, voxelBase = 0, voxelCount = 0; uint8_t inlineChunks = 0; uint64_t hash2 = 0;
    std::vector<ClodDiskLocator> groupLocators;
    struct Chunk { uint32_t w[5]; }; std::vector<Chunk> chunks;
    struct S4 { float v[4]; }; std::vector<S4> sb;
    if (!getPod(in, off, schema) || schema != kClodSchemaVersion) return false;
    if (!getPod(in, off, d.buildConfigHash) || !getVec(in, off, d.groups) || !getVec(in, off, d.segments) || !getVec(in, off, sb)) return false;
    d.segmentBounds.resize(sb.size() * 4); if (!sb.empty()) std::memcpy(d.segmentBounds.data(), sb.data(), sb.size() * 16);
    if (off + 16 > in.size()) return false;
    std::memcpy(d.objectSphere, in.data() + off, 16); off += 16;
    if (!getPod(in, off, inlineChunks)) return false;
    if (inlineChunks && !getVec(in, off, chunks)) return false;
    if (!getVec(in, off, groupLocators) || !getVec(in, off, pageLocators) || !getVec(in, off, d.groupPageReferences) || !getVec(in, off, d.groupPageReferenceOffsets)) return false;
    if (!getPod(in, off, d.trianglePageCount) || !getPod(in, off, voxelBase) || !getPod(in, off, voxelCount)) return false;
    if (!getStr(in, off, d.sourceIdentifier) || !getStr(in, off, d.primPath) || !getStr(in, off, d.subsetName) || !getPod(in, off, hash2) || !getStr(in, off, d.containerFileName)) return false;
    if (!getVec(in, off, d.nodes) || !getVec(in, off, d.lodNodeRanges) || !getVec(in, off, d.lodLevelRoots) || !getPod(in, off, d.maxDepth) || !getPod(in, off, d.maxTraversalDepth)) return false;
    return off == in.size() && voxelCount == 0;                      // voxel-LOD pages are not part of this path
}

bool writeWholeFile(const std::string& path, const std::vector<uint8_t>& bytes) { std::ofstream f(path, std::ios::binary | std::ios::trunc); if (!f) return false; f.write(reinterpret_cast<const char*>(bytes.data()), (std::streamsize)bytes.size()); return f.good(); }
bool readWholeFile(const std::string& path, std::vector<uint8_t>& bytes) {
    std::ifstream f(path, std::ios::binary | std::ios::ate); if (!f) return false;
    const std::streamoff n = f.tellg(); if (n < 0) return false;
    bytes.resize((size_t)n); f.seekg(0); if (n) f.read(reinterpret_cast<char*>(bytes.data()), n); return f.good() || n == 0;
}

// mesh `m` of a generated scene in the cache's terms (everything mesh-local, as the builder emits it)
MeshCacheData collectMeshCache(const brmi_scene& sc, uint32_t m) {
    MeshCacheData d;
    const brmi_clod_mesh_metadata& md = sc.meshMetadata[m];
    const brmi_scene::MeshCacheInfo& ci = sc.meshCache[m];
    d.groups.assign(sc.groups.begin() + md.groupsBase, sc.groups.begin() + md.groupsBase + ci.groupCount);
    d.segments.assign(sc.segments.begin() + md.segmentsBase, sc.segments.begin() + md.segmentsBase + ci.segmentCount);
    d.segmentBounds = ci.segmentBounds;
    std::memcpy(d.objectSphere, sc.perMesh[m].boundingSphere, 16);
    d.nodes.assign(sc.nodes.begin() + md.lodNodesBase, sc.nodes.begin() + md.lodNodesBase + ci.nodeCount);
    for (size_t k = 0; k + 1 < ci.lodNodeRanges.size(); k += 2) d.lodNodeRanges.push_back({ci.lodNodeRanges[k], ci.lodNodeRanges[k + 1]});
    for (uint32_t L = 0; L < md.lodLevelCount; L++) d.lodLevelRoots.push_back(1 + L);       // ClusterLODUtilities.cpp:4677-4679
    d.maxDepth = md.lodLevelCount ? md.lodLevelCount - 1 : 0; d.maxTraversalDepth = ci.maxTraversalDepth;
    d.trianglePageCount = ci.pageCount;
    for (uint32_t pg = 0; pg < ci.pageCount; pg++) {
        const brmi_group_page_map_entry& e = sc.pageMap[md.pageMapBase + pg];
        const uint8_t* base = sc.slabs[e.slabDescriptorIndex].data() + e.slabByteOffset;
        // the blob proper: up to the end of the triangle stream, the last section (BuildPackedTriangleMeshPageBlob's order)
        const brmi_page_header* h = reinterpret_cast<const brmi_page_header*>(base);
        size_t triBytes = 0;
        for (uint32_t q = 0; q < h->meshletCount; q++) { brmi_meshlet_descriptor ds; std::memcpy(&ds, base + h->descriptorOffset + (size_t)q * 64u, 64); triBytes += (size_t)(ds.triangleCountAndRefinedGroup & 0xFFFFu) * 3u; }
        d.pages.emplace_back(base, base + std::min<size_t>(BRMI_PAGE_SIZE, align4(h->triangleStreamOffset + triBytes)));
    }
    d.groupPageReferenceOffsets.push_back(0);
    for (const brmi_lod_group& g : d.groups) {                         // pages a group's segments live in
        std::vector<uint32_t> pages;
        for (uint32_t k = 0; k < g.segmentCount; k++) { const uint32_t pi = d.segments[g.firstSegment + k].pageIndex; if (std::find(pages.begin(), pages.end(), pi) == pages.end()) pages.push_back(pi); }
        d.groupPageReferences.insert(d.groupPageReferences.end(), pages.begin(), pages.end());
        d.groupPageReferenceOffsets.push_back((uint32_t)d.groupPageReferences.size());
    }
    d.sourceIdentifier = "brmi_scene"; d.primPath = "/mesh_" + std::to_string(m); d.subsetName = ""; d.containerFileName = "mesh_" + std::to_string(m) + ".clodbin";
    d.buildConfigHash = 0x62726D69ull;
    return d;
}

bool saveMeshCache(const MeshCacheData& d, const std::string& dir, uint32_t m) {
    std::vector<ClodDiskLocator> loc(d.pages.size());
    std::vector<uint8_t> file;
    const uint32_t header[4] = {kClodContainerMagic, kClodContainerVersion, 0u, (uint32_t)d.pages.size()};
    putPod(file, header);
    const size_t dirOff = file.size();
    file.resize(file.size() + loc.size() * sizeof(ClodDiskLocator), 0);
    for (size_t i = 0; i < d.pages.size(); i++) { loc[i] = {(uint64_t)file.size(), (uint32_t)d.pages[i].size(), 0u}; file.insert(file.end(), d.pages[i].begin(), d.pages[i].end()); }
    if (!loc.empty()) std::memcpy(file.data() + dirOff, loc.data(), loc.size() * sizeof(ClodDiskLocator));
    const std::string stem = dir + "/mesh_" + std::to_string(m);
    return writeWholeFile(stem + ".clodbin", file) && writeWholeFile(stem + ".clodmeta", serializeClodMetadata(d, loc));
}

bool loadMeshCache(const std::string& dir, uint32_t m, MeshCacheData& d) {
    const std::string stem = dir + "/mesh_" + std::to_string(m);
    std::vector<uint8_t> meta, file; std::vector<ClodDiskLocator> metaLoc;
    if (!readWholeFile(stem + ".clodmeta", meta) || !deserializeClodMetadata(meta, d, metaLoc)) return false;
    if (!readWholeFile(stem + ".clodbin", file) || file.size() < 16) return false;
    uint32_t header[4]; std::memcpy(header, file.data(), 16);
    if (header[0] != kClodContainerMagic || header[1] != kClodContainerVersion) return false;           // OpenContainerFile, CLodCache.cpp:1014
    const uint32_t pageCount = header[3];
    if (file.size() < 16 + (size_t)pageCount * sizeof(ClodDiskLocator) || metaLoc.size() != pageCount) return false;
    std::vector<ClodDiskLocator> loc(pageCount);
    if (pageCount) std::memcpy(loc.data(), file.data() + 16, (size_t)pageCount * sizeof(ClodDiskLocator));
    for (uint32_t i = 0; i < pageCount; i++) {
        if (loc[i].blobOffset != metaLoc[i].blobOffset || loc[i].blobSizeBytes != metaLoc[i].blobSizeBytes) return false;     // directory and metadata agree
        if (loc[i].blobOffset > file.size() || loc[i].blobSizeBytes > file.size() - loc[i].blobOffset || loc[i].blobSizeBytes > BRMI_PAGE_SIZE) return false;
        d.pages.emplace_back(file.begin() + (size_t)loc[i].blobOffset, file.begin() + (size_t)loc[i].blobOffset + loc[i].blobSizeBytes);
    }
    // the structure the kernels index without checks: validate every cross reference once, here
    if (pageCount == 0 || d.trianglePageCount != pageCount || d.nodes.empty() || d.groupPageReferenceOffsets.size() != d.groups.size() + 1) return false;
    for (const brmi_lod_segment& sg : d.segments) if (sg.pageIndex >= pageCount || sg.refinedGroup >= (int32_t)d.groups.size()) return false;
    for (const brmi_lod_group& g : d.groups) if ((uint64_t)g.firstSegment + g.segmentCount > d.segments.size()) return false;
    for (const brmi_lod_node& n : d.nodes) {
        if (n.isLeaf == BRMI_NODE_INTERNAL) { if ((uint64_t)n.indexOrOffset + n.countMinusOne + 1 > d.nodes.size() || n.countMinusOne + 1 > BRMI_BVH_MAX_CHILDREN) return false; }
        else if (n.indexOrOffset >= d.segments.size() || n.ownerGroupId >= d.groups.size()) return false;
    }
    for (size_t si = 0; si < d.segments.size(); si++) {
        const std::vector<uint8_t>& pg = d.pages[d.segments[si].pageIndex];
        if (pg.size() < sizeof(brmi_page_header)) return false;
        const brmi_page_header* h = reinterpret_cast<const brmi_page_header*>(pg.data());
        if ((uint64_t)d.segments[si].firstMeshletInPage + d.segments[si].meshletCount > h->meshletCount || (uint64_t)h->descriptorOffset + (uint64_t)h->meshletCount * 64u > pg.size()) return false;
    }
    return true;
}

// buildMesh's emission from cached data: the same appends, with the material / skinning flags of the mesh definition
bool loadCachedMesh(brmi_scene& sc, const MeshDef& def, uint32_t meshIndex) {
    MeshCacheData d;
    if (!loadMeshCache(sc.cacheDir, meshIndex, d)) return false;
    const uint32_t pageMapBase = (uint32_t)sc.pageMap.size(), groupsBase = (uint32_t)sc.groups.size(), segmentsBase = (uint32_t)sc.segments.size(), nodesBase = (uint32_t)sc.nodes.size();
    for (auto& pg : d.pages) sc.pageMap.push_back(allocPage(sc, pg));
    sc.groups.insert(sc.groups.end(), d.groups.begin(), d.groups.end());
    sc.segments.insert(sc.segments.end(), d.segments.begin(), d.segments.end());
    sc.nodes.insert(sc.nodes.end(), d.nodes.begin(), d.nodes.end());
    const uint32_t levels = (uint32_t)d.lodLevelRoots.size();
    brmi_scene::MeshCacheInfo ci;
    ci.groupCount = (uint32_t)d.groups.size(); ci.segmentCount = (uint32_t)d.segments.size(); ci.nodeCount = (uint32_t)d.nodes.size(); ci.pageCount = (uint32_t)d.pages.size();
    ci.maxTraversalDepth = d.maxTraversalDepth; ci.segmentBounds = d.segmentBounds;
    for (const ClodNodeRange& r : d.lodNodeRanges) { ci.lodNodeRanges.push_back(r.offset); ci.lodNodeRanges.push_back(r.count); }
    sc.meshCache.push_back(std::move(ci));
    brmi_clod_mesh_metadata md{};
    md.groupsBase = groupsBase; md.segmentsBase = segmentsBase; md.lodNodesBase = nodesBase; md.rootNode = 0;
    md.pageMapBase = pageMapBase; md.lodLevelCount = levels; md.maxDepth = d.maxTraversalDepth;
    sc.meshMetadata.push_back(md);
    // meshlet statistics of the finest level from the pages themselves
    uint32_t total = 0, lod0 = 0, lod0Verts = 0; uint64_t lod0Tris = 0;
    for (const brmi_lod_group& g : d.groups) {
        total += g.meshletCount;
        if (g.depth != 0) continue;
        for (uint32_t k = 0; k < g.segmentCount; k++) {
            const brmi_lod_segment& sg = d.segments[g.firstSegment + k];
            const std::vector<uint8_t>& pg = d.pages[sg.pageIndex];
            const brmi_page_header* h = reinterpret_cast<const brmi_page_header*>(pg.data());
            for (uint32_t q = 0; q < sg.meshletCount; q++) {
                brmi_meshlet_descriptor ds; std::memcpy(&ds, pg.data() + h->descriptorOffset + (size_t)(sg.firstMeshletInPage + q) * 64u, 64);
                lod0++; lod0Verts += (ds.bitsAndVertexCount >> 24) & 0xFFu; lod0Tris += ds.triangleCountAndRefinedGroup & 0xFFFFu;
            }
        }
    }
    brmi_per_mesh pm{};
    pm.materialDataIndex = def.material; pm.rasterBucketIndex = 0;
    const brmi_page_header* h0 = reinterpret_cast<const brmi_page_header*>(d.pages[0].data());
    pm.vertexFlags = (1u << 1) | (def.skinned ? BRMI_VERTEX_SKINNED : 0u) | ((h0->attributeMask & BRMI_PAGE_ATTRIBUTE_COLOR) ? 1u : 0u) | (h0->uvSetCount ? (1u << 2) : 0u);
    pm.vertexByteSize = 24;
    std::memcpy(pm.boundingSphere, d.objectSphere, 16);
    pm.clodNumMeshlets = total; pm.numMeshlets = lod0; pm.numVertices = lod0Verts;
    sc.perMesh.push_back(pm);
    sc.meshLod0Triangles.push_back(lod0Tris);
    sc.stats.meshletsTotal += total; sc.stats.meshletsLod0 += lod0; sc.stats.uniqueTriangles += lod0Tris;
    sc.stats.maxBvhDepth = std::max(sc.stats.maxBvhDepth, d.maxTraversalDepth);
    sc.stats.lodLevelsMax = std::max(sc.stats.lodLevelsMax, levels);
    return true;
}

void addInstance(brmi_scene& sc, const InstanceDef& instIn) {
    InstanceDef inst = instIn;
    // materialFeatures bit 2: every third instance (not the first: usually the ground) is mirrored in its local x axis and drawn with
    // reversed winding (negative-determinant transforms, BRMI_OBJECT_FLAG_REVERSE_WINDING)
    if ((sc.params.materialFeatures & 4u) && sc.perMeshInstance.size() % 3u == 2u) {
        M4 mirror = identity(); mirror.m[0][0] = -1.0;
        inst.model = mul(mirror, inst.model);
        inst.reverseWinding = !inst.reverseWinding;
    }
    brmi_per_object o{};
    store(o.model, inst.model); store(o.prevModel, inst.model); store(o.modelInverse, inverse(inst.model));
    o.normalMatrixBufferIndex = (uint32_t)sc.perObject.size();
    o.objectFlags = inst.reverseWinding ? BRMI_OBJECT_FLAG_REVERSE_WINDING : 0u;
    M4 nm = transpose(inverse(inst.model));
    nm.m[0][3] = nm.m[1][3] = nm.m[2][3] = 0; nm.m[3][0] = nm.m[3][1] = nm.m[3][2] = 0; nm.m[3][3] = 1;
    float nmf[4][4]; store(nmf, nm);
    sc.normalMatrices.insert(sc.normalMatrices.end(), &nmf[0][0], &nmf[0][0] + 16);
    brmi_per_mesh_instance mi{};
    mi.perMeshBufferIndex = inst.mesh; mi.perObjectBufferIndex = (uint32_t)sc.perObject.size();
    mi.skinningInstanceSlot = inst.skinSlot; mi.skinnedBoundsScale = 1.0f;
    std::memcpy(mi.boundingSphere, sc.perMesh[inst.mesh].boundingSphere, 16);
    sc.activeDraws.push_back((uint32_t)sc.perMeshInstance.size());
    sc.perMeshInstance.push_back(mi);
    sc.clodOffsets.push_back({inst.mesh});
    sc.perObject.push_back(o);
    sc.stats.instancedTriangles += sc.meshLod0Triangles[inst.mesh];
    // scene bounds
    const float* bs = sc.perMesh[inst.mesh].boundingSphere;
    V3 c = xformPoint({bs[0], bs[1], bs[2]}, inst.model);
    double sx = std::sqrt(inst.model.m[0][0] * inst.model.m[0][0] + inst.model.m[0][1] * inst.model.m[0][1] + inst.model.m[0][2] * inst.model.m[0][2]);
    double r = bs[3] * sx;
    for (int k = 0; k < 3; k++) {
        double cv = k == 0 ? c.x : (k == 1 ? c.y : c.z);
        sc.stats.sceneMin[k] = std::min(sc.stats.sceneMin[k], (float)(cv - r));
        sc.stats.sceneMax[k] = std::max(sc.stats.sceneMax[k], (float)(cv + r));
    }
}

// ---- procedural textures (materialFeatures bits 3 / 4) ----------------------------------------------------------------
// RGBA8 with a full box-filtered mip chain.  kind 0: base colour (sRGB) with an alpha mask of round holes; 1: occlusion (R) /
// roughness (G) / metallic (B), linear; 2: tangent-space normal map; 3: emissive (sRGB) sparse dots; 4: opacity (A) stripes;
// 5: height map (R): bricks above their mortar, fbm on top; 6: the same a twentieth as tall (view rays mostly never dip below it).
uint32_t addTexture(brmi_scene& sc, uint32_t kind, uint32_t size, uint32_t seed) {
    brmi_texture_desc d{};
    d.texels = reinterpret_cast<const uint8_t*>((uintptr_t)sc.texels.size());
    d.width = size; d.height = size; d.format = (kind == 0 || kind == 3) ? BRMI_TEXTURE_FORMAT_RGBA8_UNORM_SRGB : BRMI_TEXTURE_FORMAT_RGBA8_UNORM;
    std::vector<float> lvl((size_t)size * size * 4);
    auto q8 = [](double x) { return (uint8_t)std::lround(std::max(0.0, std::min(1.0, x)) * 255.0); };
    for (uint32_t y = 0; y < size; y++) for (uint32_t x = 0; x < size; x++) {
        const double u = (x + 0.5) / size, v = (y + 0.5) / size;
        float* t = &lvl[((size_t)y * size + x) * 4];
        const double n = fbm(u * 8.0, v * 8.0, seed), n2 = fbm(u * 16.0 + 3.0, v * 16.0 + 7.0, seed ^ 0x9E37u);
        if (kind == 0) {
            const bool brick = (((int)(v * 8.0) & 1) ? std::fmod(u * 4.0 + 0.5, 1.0) : std::fmod(u * 4.0, 1.0)) < 0.06 || std::fmod(v * 8.0, 1.0) < 0.1;
            const double base = brick ? 0.35 : 0.75;
            t[0] = (float)(base + 0.25 * n); t[1] = (float)(base * 0.9 + 0.2 * n2); t[2] = (float)(base * 0.8 + 0.15 * n);
            // alpha: 4x4 round holes with a soft edge (the cutoff of an alpha-tested material cuts through the gradient)
            const double cx = std::fmod(u * 4.0, 1.0) - 0.5, cy = std::fmod(v * 4.0, 1.0) - 0.5, r = std::sqrt(cx * cx + cy * cy);
            t[3] = (float)std::max(0.0, std::min(1.0, (r - 0.22) * 10.0 + 0.5));
        } else if (kind == 1) {
            t[0] = (float)(0.6 + 0.4 * n); t[1] = (float)(0.2 + 0.8 * n2); t[2] = (float)((std::fmod(u * 6.0, 1.0) < 0.5) == (std::fmod(v * 6.0, 1.0) < 0.5) ? 0.9 : 0.05); t[3] = 1.0f;
        } else if (kind == 2) {
            const double e = 1.0 / size;
            const double hx = fbm((u + e) * 8.0, v * 8.0, seed) - fbm((u - e) * 8.0, v * 8.0, seed), hy = fbm(u * 8.0, (v + e) * 8.0, seed) - fbm(u * 8.0, (v - e) * 8.0, seed);
            V3 nn = normalize(V3{-hx * 24.0, -hy * 24.0, 1.0});
            t[0] = (float)(nn.x * 0.5 + 0.5); t[1] = (float)(nn.y * 0.5 + 0.5); t[2] = (float)(nn.z * 0.5 + 0.5); t[3] = 1.0f;
        } else if (kind == 3) {
            const double cx = std::fmod(u * 6.0, 1.0) - 0.5, cy = std::fmod(v * 6.0, 1.0) - 0.5;
            const double g = std::max(0.0, 1.0 - std::sqrt(cx * cx + cy * cy) * 5.0);
            t[0] = (float)g; t[1] = (float)(g * (0.4 + 0.6 * n)); t[2] = (float)(g * 0.3); t[3] = 1.0f;
        } else if (kind == 5 || kind == 6) {
            const bool mortar = (((int)(v * 8.0) & 1) ? std::fmod(u * 4.0 + 0.5, 1.0) : std::fmod(u * 4.0, 1.0)) < 0.06 || std::fmod(v * 8.0, 1.0) < 0.1;
            const double h = (mortar ? 0.15 : 0.7) + 0.3 * n;
            t[0] = t[1] = t[2] = (float)(kind == 6 ? h * 0.05 : h); t[3] = 1.0f;
        } else {
            t[0] = t[1] = t[2] = 1.0f;
            t[3] = (float)std::max(0.0, std::min(1.0, (std::fabs(std::fmod(u * 5.0 + v * 2.0, 1.0) - 0.5) - 0.15) * 8.0 + 0.5));
        }
    }
    uint32_t w = size, offsetTexels = 0, level = 0;
    for (;;) {
        d.mipOffset[level] = offsetTexels;
        for (size_t k = 0; k < (size_t)w * w * 4; k++) sc.texels.push_back(q8(lvl[k]));
        offsetTexels += w * w; level++;
        if (w == 1) break;
        const uint32_t h2 = w / 2;
        std::vector<float> nxt((size_t)h2 * h2 * 4);
        for (uint32_t y = 0; y < h2; y++) for (uint32_t x = 0; x < h2; x++) for (int c = 0; c < 4; c++)
            nxt[((size_t)y * h2 + x) * 4 + c] = 0.25f * (lvl[((size_t)(2 * y) * w + 2 * x) * 4 + c] + lvl[((size_t)(2 * y) * w + 2 * x + 1) * 4 + c] +
                                                        lvl[((size_t)(2 * y + 1) * w + 2 * x) * 4 + c] + lvl[((size_t)(2 * y + 1) * w + 2 * x + 1) * 4 + c]);
        lvl.swap(nxt); w = h2;
    }
    d.mipCount = level;
    sc.textureDescs.push_back(d);
    return (uint32_t)sc.textureDescs.size() - 1;
}

struct TextureSet { std::vector<uint32_t> base, orm, normal, emissive, opacity, height; };
TextureSet addTextures(brmi_scene& sc) {
    // samplers: the reference's default (Sampler.cpp:20-40: trilinear, wrap), a clamp / mirror one, linear with nearest mip, all point
    sc.samplerDescs.push_back({BRMI_ADDRESS_WRAP, BRMI_ADDRESS_WRAP, BRMI_FILTER_LINEAR, BRMI_FILTER_LINEAR, BRMI_FILTER_LINEAR, 0.0f, 0.0f, FLT_MAX});
    sc.samplerDescs.push_back({BRMI_ADDRESS_CLAMP, BRMI_ADDRESS_MIRROR, BRMI_FILTER_LINEAR, BRMI_FILTER_LINEAR, BRMI_FILTER_LINEAR, 0.0f, 0.0f, FLT_MAX});
    sc.samplerDescs.push_back({BRMI_ADDRESS_WRAP, BRMI_ADDRESS_WRAP, BRMI_FILTER_LINEAR, BRMI_FILTER_LINEAR, BRMI_FILTER_POINT, 0.5f, 0.0f, 6.0f});
    sc.samplerDescs.push_back({BRMI_ADDRESS_MIRROR, BRMI_ADDRESS_WRAP, BRMI_FILTER_POINT, BRMI_FILTER_POINT, BRMI_FILTER_POINT, 0.0f, 1.0f, FLT_MAX});
    sc.srgbToLinear.resize(256);
    for (int c = 0; c < 256; c++) { const double x = c / 255.0; sc.srgbToLinear[c] = (float)(x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4)); }
    TextureSet t;
    const uint32_t seed = 0x7E57u + sc.params.seed;
    const uint32_t sizes[4] = {256, 128, 512, 64};
    for (uint32_t k = 0; k < 4; k++) t.base.push_back(addTexture(sc, 0, sizes[k], seed + k));
    for (uint32_t k = 0; k < 2; k++) t.orm.push_back(addTexture(sc, 1, sizes[k], seed + 16 + k));
    for (uint32_t k = 0; k < 2; k++) t.normal.push_back(addTexture(sc, 2, sizes[k], seed + 32 + k));
    t.emissive.push_back(addTexture(sc, 3, 128, seed + 48));
    t.opacity.push_back(addTexture(sc, 4, 128, seed + 64));
    if (sc.params.materialFeatures & 128u) { t.height.push_back(addTexture(sc, 5, 256, seed + 80)); t.height.push_back(addTexture(sc, 5, 128, seed + 81)); t.height.push_back(addTexture(sc, 6, 64, seed + 82)); }
    return t;
}

void addMaterials(brmi_scene& sc, Pcg32& rng, uint32_t count) {
    const bool textured = (sc.params.materialFeatures & 24u) != 0u, alphaTested = (sc.params.materialFeatures & 16u) != 0u;
    TextureSet tex;
    if (textured) tex = addTextures(sc);
    for (uint32_t i = 0; i < count; i++) {
        brmi_material_info m{};
        std::memset(&m, 0, sizeof(m));
        m.materialFlags = 0;
        bool metal = (i % 5) == 3;
        bool emissive = (i % 11) == 7;
        m.metallicFactor = metal ? 1.0f : 0.0f;
        m.roughnessFactor = rng.range(0.25f, 0.9f);
        m.ambientStrength = 1.0f; m.specularStrength = 1.0f; m.textureScale = 1.0f; m.alphaCutoff = 0.5f;
        m.baseColorFactor[0] = rng.range(0.15f, 0.95f); m.baseColorFactor[1] = rng.range(0.15f, 0.95f); m.baseColorFactor[2] = rng.range(0.15f, 0.95f); m.baseColorFactor[3] = 1.0f;
        if (emissive) { m.emissiveFactor[0] = rng.range(0.0f, 2.0f); m.emissiveFactor[1] = rng.range(0.0f, 2.0f); m.emissiveFactor[2] = rng.range(0.0f, 2.0f); }
        m.emissiveFactor[3] = 1.0f;
        m.compileFlagsID = 0; m.rasterBucketIndex = 0; m.openPBRMaterialDataIndex = i;
        m.baseColorChannels[0] = 0; m.baseColorChannels[1] = 1; m.baseColorChannels[2] = 2; m.baseColorChannels[3] = 3;
        m.normalChannels[0] = 0; m.normalChannels[1] = 1; m.normalChannels[2] = 2;
        m.emissiveChannels[0] = 0; m.emissiveChannels[1] = 1; m.emissiveChannels[2] = 2;
        if (textured && (i % 4) != 3) {           // every fourth material stays constant-factor
            m.materialFlags |= BRMI_MATERIAL_TEXTURED | BRMI_MATERIAL_BASE_COLOR_TEXTURE;
            m.baseColorTextureIndex = tex.base[i % tex.base.size()]; m.baseColorSamplerIndex = (i / 4) % 4u;
            m.baseColorFactor[0] = m.baseColorFactor[0] * 0.5f + 0.5f; m.baseColorFactor[1] = m.baseColorFactor[1] * 0.5f + 0.5f; m.baseColorFactor[2] = m.baseColorFactor[2] * 0.5f + 0.5f;
            if ((i % 2) == 0) {                  // glTF packing: occlusion R, roughness G, metallic B of one texture
                m.materialFlags |= BRMI_MATERIAL_METALLIC_TEXTURE | BRMI_MATERIAL_ROUGHNESS_TEXTURE;
                m.metallicTextureIndex = m.roughnessTextureIndex = tex.orm[(i / 2) % tex.orm.size()];
                m.metallicSamplerIndex = m.roughnessSamplerIndex = 0; m.metallicChannel = 2; m.roughnessChannel = 1;
                m.metallicFactor = 1.0f; m.roughnessFactor = 1.0f;
                if ((i % 3) == 0) { m.materialFlags |= BRMI_MATERIAL_AO_TEXTURE; m.aoMapIndex = m.metallicTextureIndex; m.aoSamplerIndex = 0; m.aoChannel = 0; }
            }
            if ((i % 3) != 1) {
                m.materialFlags |= BRMI_MATERIAL_NORMAL_MAP; m.normalTextureIndex = tex.normal[i % tex.normal.size()]; m.normalSamplerIndex = (i % 5) == 0 ? 1u : 0u;
                if ((i % 7) == 2) m.materialFlags |= BRMI_MATERIAL_INVERT_NORMAL_GREEN;
            }
            if ((i % 5) == 2) {
                m.materialFlags |= BRMI_MATERIAL_EMISSIVE_TEXTURE; m.emissiveTextureIndex = tex.emissive[0]; m.emissiveSamplerIndex = 0;
                m.emissiveFactor[0] = 1.5f; m.emissiveFactor[1] = 1.0f; m.emissiveFactor[2] = 0.5f;
            }
        }
        // materialFeatures bit 7 (with bit 3): parallax on about half of the textured materials, with and without a normal map
        if ((sc.params.materialFeatures & 128u) && (m.materialFlags & BRMI_MATERIAL_TEXTURED) && ((i % 2) == 1 || (i % 6) == 0)) {
            m.materialFlags |= BRMI_MATERIAL_PARALLAX;
            m.heightMapIndex = tex.height[i % tex.height.size()]; m.heightSamplerIndex = (i % 4) == 1 ? 2u : 0u;
            m.heightMapScale = 0.02f + 0.01f * (float)(i % 7);
        }
        // materialFeatures bit 8 (with bit 3): texture slots spread over the pages' three UV sets -- packed slots sharing a set, the normal map (and with it
        // the tangent frame) on its own set, the height map on a set only some slots share, an index past the page's sets (reads (0, 0)) and one >= 8 (reads set 0)
        if ((sc.params.materialFeatures & 256u) && (m.materialFlags & BRMI_MATERIAL_TEXTURED)) {
            switch (i % 5) {
                case 0: m.aoUvSetIndex = 1; m.metallicUvSetIndex = 1; m.roughnessUvSetIndex = 1; m.emissiveUvSetIndex = 2; break;
                case 1: m.normalUvSetIndex = 1; m.heightUvSetIndex = 1; m.baseColorUvSetIndex = 1; break;
                case 2: m.baseColorUvSetIndex = 2; m.emissiveUvSetIndex = 1; m.normalUvSetIndex = 2; break;
                case 3: m.heightUvSetIndex = 2; m.baseColorUvSetIndex = 2; m.metallicUvSetIndex = 1; m.roughnessUvSetIndex = 2; break;
                default: m.baseColorUvSetIndex = 9; m.metallicUvSetIndex = 3; m.roughnessUvSetIndex = 3; m.aoUvSetIndex = 1; break;
            }
        }
        if (alphaTested && (i % 3) == 0) {
            m.materialFlags |= BRMI_MATERIAL_ALPHA_TEST | BRMI_MATERIAL_TEXTURED | BRMI_MATERIAL_BASE_COLOR_TEXTURE;
            m.baseColorTextureIndex = tex.base[i % tex.base.size()]; m.baseColorSamplerIndex = (i / 3) % 3u;     // linear-filtered samplers cut through the soft edge
            m.alphaCutoff = 0.35f + 0.05f * (float)(i % 5);
            if ((i % 2) == 0) { m.materialFlags |= BRMI_MATERIAL_OPACITY_TEXTURE; m.opacityTextureIndex = tex.opacity[0]; m.opacitySamplerIndex = 0; }
        }
        sc.materials.push_back(m);
        brmi_openpbr_material_info o{};
        std::memset(&o, 0, sizeof(o));
        o.baseWeight = 1.0f; o.baseColor[0] = m.baseColorFactor[0]; o.baseColor[1] = m.baseColorFactor[1]; o.baseColor[2] = m.baseColorFactor[2];
        o.baseDiffuseRoughness = (i % 3 == 0) ? rng.range(0.0f, 0.6f) : 0.0f;
        o.baseMetalness = m.metallicFactor;
        o.specularWeight = 1.0f; o.specularColor[0] = o.specularColor[1] = o.specularColor[2] = 1.0f;
        o.specularRoughness = m.roughnessFactor; o.specularIor = 1.5f; o.specularAnisotropyRotationCosSin[0] = 1.0f;
        o.coatWeight = 0.0f; o.coatColor[0] = o.coatColor[1] = o.coatColor[2] = 1.0f; o.coatRoughness = 0.0f; o.coatIor = 1.6f; o.coatDarkening = 1.0f;
        o.coatAnisotropyRotationCosSin[0] = 1.0f;
        o.fuzzWeight = 0.0f; o.fuzzColor[0] = o.fuzzColor[1] = o.fuzzColor[2] = 1.0f; o.fuzzRoughness = 0.5f;
        o.transmissionColor[0] = o.transmissionColor[1] = o.transmissionColor[2] = 1.0f;
        if ((sc.params.materialFeatures & 1u) && (i % 3) == 1) {
            o.coatWeight = rng.range(0.3f, 1.0f); o.coatRoughness = rng.range(0.0f, 0.4f); o.coatDarkening = rng.range(0.0f, 1.0f);
            o.coatColor[0] = rng.range(0.6f, 1.0f); o.coatColor[1] = rng.range(0.6f, 1.0f); o.coatColor[2] = rng.range(0.6f, 1.0f);
            if (i % 2) o.coatRoughness = 0.0f;
        }
        if ((sc.params.materialFeatures & 2u) && (i % 3) == 2) {
            o.fuzzWeight = rng.range(0.2f, 1.0f); o.fuzzRoughness = rng.range(0.1f, 0.9f);
            o.fuzzColor[0] = rng.range(0.3f, 1.0f); o.fuzzColor[1] = rng.range(0.3f, 1.0f); o.fuzzColor[2] = rng.range(0.3f, 1.0f);
        }
        o.thinFilmIor = 1.4f; o.emissionLuminance = 0.0f; o.geometryOpacity = 1.0f;
        // coat / fuzz texture + sampler indices (words 0-11 of the binding tail): OPENPBR_INVALID_TEXTURE_INDEX = no texture (utilities.hlsli:641-646);
        // colour channels 0,1,2,3 as the reference's defaults
        for (int k = 0; k < 12; k++) o.textureBindings[k] = 0xFFFFFFFFu;
        for (int k = 0; k < 4; k++) { o.textureBindings[12 + k] = (uint32_t)k; o.textureBindings[19 + k] = (uint32_t)k; }
        // materialFeatures bit 6 (with bit 3 for the UVs): layered materials also texture their coat / fuzz parameters
        if ((sc.params.materialFeatures & 64u) && textured) {
            if (o.coatWeight > 0.0f) {
                o.textureBindings[0] = tex.base[(i + 1) % tex.base.size()]; o.textureBindings[1] = 0;                 // coat colour (sRGB)
                o.textureBindings[2] = tex.orm[i % tex.orm.size()]; o.textureBindings[3] = 0; o.textureBindings[16] = 0;      // coat weight: R of the ORM texture
                if (i % 2) { o.textureBindings[4] = tex.orm[(i + 1) % tex.orm.size()]; o.textureBindings[5] = 2; o.textureBindings[17] = 1; o.coatRoughness = 0.6f; }   // coat roughness: G
            }
            if (o.fuzzWeight > 0.0f) {
                o.textureBindings[6] = tex.base[(i + 2) % tex.base.size()]; o.textureBindings[7] = 1; o.textureBindings[19] = 2; o.textureBindings[21] = 0;   // fuzz colour, b / g / r
                o.textureBindings[8] = tex.orm[i % tex.orm.size()]; o.textureBindings[9] = 0; o.textureBindings[23] = 1;      // fuzz weight: G
                o.textureBindings[10] = tex.orm[i % tex.orm.size()]; o.textureBindings[11] = 0; o.textureBindings[24] = 0;    // fuzz roughness: R (same binding: one fetch)
            }
        }
        if ((sc.params.materialFeatures & 256u) && textured) {      // bit 8: the coat weight and fuzz colour slots on other UV sets (textureBindings[26..31] = the slots' set indices)
            o.textureBindings[26 + 1] = 1; o.textureBindings[26 + 3] = 2; if (i % 2) o.textureBindings[26 + 5] = 1;
        }
        sc.openpbr.push_back(o);
    }
}

// BR/src/Utilities/MathUtils.cpp:36-69
float calculateLightRadius(float intensity, float constant, float linear, float quadratic, float threshold = 0.3f) {
    float a = quadratic, b = linear;
    float c = constant - (intensity / threshold);
    float d = 0.0f;
    if (std::fabs(a) > 1e-6f) {
        float disc = (float)(b * b - 4.0 * a * c);
        d = disc < 0.0f ? 0.0f : (-b + std::sqrt(disc)) / (2.0f * a);
    } else if (std::fabs(b) > 1e-6f) d = -c / b;
    return d;
}

// BR/src/Scene/Scene.cpp:219-262
void addLight(brmi_scene& sc, uint32_t type, V3 pos, V3 color, float intensity, V3 att, V3 dir) {
    // spot lights on request: every spotLightEvery-th point light becomes a spot aimed roughly at the scene floor
    // (BR/src/Scene/Scene.cpp:220-262: cone angles stored as cosines, bounding sphere of the cone from MathUtils.cpp:70-82)
    double innerAngle = 0.0, outerAngle = 0.0;
    if (type == BRMI_LIGHT_POINT && sc.params.spotLightEvery != 0 && (sc.lights.size() % sc.params.spotLightEvery) == 0) {
        type = BRMI_LIGHT_SPOT;
        const double k = (double)(sc.lights.size() % 7) / 7.0;
        dir = V3{0.6 * std::cos(6.2831 * k), -1.0, 0.6 * std::sin(6.2831 * k)};
        innerAngle = 0.35 + 0.2 * k; outerAngle = innerAngle + 0.25;
    }
    brmi_light_info l{};
    std::memset(&l, 0, sizeof(l));
    V3 an = normalize(att);
    float maxRange = calculateLightRadius(intensity, (float)an.x, (float)an.y, (float)an.z);
    l.type = type;
    l.posWorldSpace[0] = (float)pos.x; l.posWorldSpace[1] = (float)pos.y; l.posWorldSpace[2] = (float)pos.z; l.posWorldSpace[3] = 0.0f;
    V3 cn = normalize(color);
    l.color[0] = (float)cn.x; l.color[1] = (float)cn.y; l.color[2] = (float)cn.z; l.color[3] = intensity;
    l.attenuation[0] = (float)an.x; l.attenuation[1] = (float)an.y; l.attenuation[2] = (float)an.z; l.attenuation[3] = 0.0f;
    V3 dn = (type == BRMI_LIGHT_POINT) ? V3{0, 0, 0} : normalize(dir);
    l.dirWorldSpace[0] = (float)dn.x; l.dirWorldSpace[1] = (float)dn.y; l.dirWorldSpace[2] = (float)dn.z;
    l.innerConeAngle = (float)std::cos(innerAngle); l.outerConeAngle = (float)std::cos(outerAngle);   // cos(0) = 1 for non-spot lights
    l.shadowViewInfoIndex = -1; l.nearPlane = 0.01f; l.farPlane = maxRange;
    l.shadowMapIndex = -1; l.shadowSamplerIndex = -1; l.shadowCaster = 0;
    l.maxRange = maxRange;
    if (type == BRMI_LIGHT_POINT) { l.boundingSphere[0] = (float)pos.x; l.boundingSphere[1] = (float)pos.y; l.boundingSphere[2] = (float)pos.z; l.boundingSphere[3] = maxRange; }
    if (type == BRMI_LIGHT_SPOT) {      // ComputeConeBoundingSphere(origin, direction, height = maxRange, halfAngle = outer)
        const float r = maxRange * std::tan((float)outerAngle);
        const V3 c = pos + dn * (0.5 * (double)maxRange);
        l.boundingSphere[0] = (float)c.x; l.boundingSphere[1] = (float)c.y; l.boundingSphere[2] = (float)c.z; l.boundingSphere[3] = std::sqrt(maxRange * maxRange + r * r);
    }
    sc.activeLights.push_back((uint32_t)sc.lights.size());
    sc.lights.push_back(l);
}

// BR/src/Scene/Scene.cpp:509-535 (SetCamera) + ViewManager.cpp:19-77 (culling camera)
// `step` / `prevStep`: position on the camera path (whole numbers = the test frames; brmi_scene_camera_at walks it in fractions)
void makeCamera(uint32_t W, uint32_t H, V3 eye, double yaw, double pitch, double fovDeg, double zNear, double zFar, double step, double prevStep,
                brmi_camera& c, brmi_culling_camera& cc) {
    const double fov = fovDeg * (M_PI / 180.0), aspect = (double)W / (double)H;
    // camera world transform (row-vector): rotate then translate ; view = inverse
    // camera path for multi-frame tests: every step strafes, advances and turns a little; prevView = view of the previous step
    auto worldAt = [&](double k) {
        const V3 e{eye.x + 0.35 * k, eye.y + 0.05 * k, eye.z - 0.6 * k};
        return mul(mul(rotationX(pitch), rotationY(yaw + 0.07 * k)), translation(e));
    };
    // (the eye moves first and the view matrices start from the moved eye: the path of the matrices is twice as long as that of
    // positionWorldSpace.  Kept as rounds 1-2 had it: the golden fixtures are frames of this path)
    { const double k = step; eye = V3{eye.x + 0.35 * k, eye.y + 0.05 * k, eye.z - 0.6 * k}; }
    M4 world = worldAt(step);
    M4 view = inverse(world);
    M4 prevView = prevStep != step ? inverse(worldAt(prevStep)) : view;
    // XMMatrixPerspectiveFovRH(fov, aspect, NearZ = zFar, FarZ = zNear): reversed Z
    M4 proj{};
    const double h = std::cos(0.5 * fov) / std::sin(0.5 * fov), w = h / aspect;
    const double nearZ = zFar, farZ = zNear, fRange = farZ / (nearZ - farZ);
    proj.m[0][0] = w; proj.m[1][1] = h; proj.m[2][2] = fRange; proj.m[2][3] = -1.0; proj.m[3][2] = fRange * nearZ;
    std::memset(&c, 0, sizeof(c));
    c.positionWorldSpace[0] = (float)eye.x; c.positionWorldSpace[1] = (float)eye.y; c.positionWorldSpace[2] = (float)eye.z; c.positionWorldSpace[3] = 1.0f;
    store(c.view, view); store(c.viewInverse, world); store(c.projection, proj); store(c.projectionInverse, inverse(proj));
    store(c.viewProjection, mul(view, proj)); store(c.prevView, prevView); store(c.prevJitteredProjection, proj);
    store(c.prevUnjitteredProjection, proj); store(c.unjitteredProjection, proj);
    // BR/src/Utilities/Utilities.cpp:1840-1868: near, far, left, right, bottom, top (view space, normalised)
    const double t = std::tan(fov / 2.0);
    double pl[6][4] = {{0, 0, -1, -zNear}, {0, 0, 1, zFar}, {1, 0, -t * aspect, 0}, {-1, 0, -t * aspect, 0}, {0, 1, -t, 0}, {0, -1, -t, 0}};
    for (int i = 0; i < 6; i++) {
        double len = std::sqrt(pl[i][0] * pl[i][0] + pl[i][1] * pl[i][1] + pl[i][2] * pl[i][2]);
        for (int k = 0; k < 4; k++) c.clippingPlanes[i][k] = (float)(pl[i][k] / len);
    }
    c.fov = (float)fov; c.aspectRatio = (float)aspect; c.zNear = (float)zNear; c.zFar = (float)zFar;
    c.depthBufferArrayIndex = -1; c.depthResX = W; c.depthResY = H;
    uint32_t mips = 1; { uint32_t m = std::max(W, H); while (m > 1) { m >>= 1; mips++; } }
    c.numDepthMips = mips; c.isOrtho = 0;
    auto nextPow2 = [](uint32_t v) { uint32_t p = 1; while (p < v) p <<= 1; return p; };
    c.UVScaleToNextPowerOf2[0] = (float)W / (float)nextPow2(W); c.UVScaleToNextPowerOf2[1] = (float)H / (float)nextPow2(H);
    std::memset(&cc, 0, sizeof(cc));
    std::memcpy(cc.positionWorldSpace, c.positionWorldSpace, 16);
    cc.projX = c.projection[0][0]; cc.projY = c.projection[1][1]; cc.zNear = c.zNear;
    { float denom = (cc.projY * 0.5f) * (float)H; cc.errorOverDistanceThreshold = denom <= 0.0f ? FLT_MAX : 1.0f / denom; }
    cc.isOrtho = 0;
    for (int k = 0; k < 3; k++) { cc.viewRightWorld[k] = c.viewInverse[0][k]; cc.viewUpWorld[k] = c.viewInverse[1][k]; cc.viewForwardWorld[k] = -c.viewInverse[2][k]; }
    std::memcpy(cc.viewProjection, c.viewProjection, 64);
    for (int k = 0; k < 4; k++) cc.viewZ[k] = c.view[k][2];
    std::memcpy(cc.viewInverse, c.viewInverse, 64); std::memcpy(cc.projectionInverse, c.projectionInverse, 64);
}

void setCamera(brmi_scene& sc, V3 eye, double yaw, double pitch, double fovDeg, double zNear, double zFar) {
    const uint32_t W = sc.params.width, H = sc.params.height;
    brmi_camera c{}; brmi_culling_camera cc{};
    const uint32_t step = sc.params.cameraStep;
    makeCamera(W, H, eye, yaw, pitch, fovDeg, zNear, zFar, (double)step, step > 0 ? (double)(step - 1) : (double)step, c, cc);
    sc.cameras.push_back(c);
    sc.cullingCameras.push_back(cc);
    brmi_view_raster_info ri{};
    ri.scissorMinX = 0; ri.scissorMinY = 0; ri.scissorMaxX = W; ri.scissorMaxY = H; ri.viewportScaleX = 1.0f; ri.viewportScaleY = 1.0f;
    sc.viewRasterInfo.push_back(ri);
}

// where each preset's camera path starts (eye, yaw, pitch); field of view 80 degrees, zNear 0.1, zFar 1000 (BasicRenderer.cpp:417-428)
bool presetCameraBase(uint32_t preset, V3& eye, double& yaw, double& pitch) {
    switch (preset) {
        case BRMI_PRESET_TINY: eye = {0.2, 1.2, 3.0}; yaw = 0.08; pitch = -0.28; return true;
        case BRMI_PRESET_SPONZA: eye = {0.6, 1.7, 16.0}; yaw = 0.10; pitch = -0.04; return true;
        case BRMI_PRESET_BISTRO: case BRMI_PRESET_SAN_MIGUEL: eye = {0.8, 1.7, 28.0}; yaw = 0.06; pitch = -0.03; return true;
        case BRMI_PRESET_ZORAH: eye = {0.0, 6.0, 20.0}; yaw = 0.0; pitch = -0.12; return true;
        default: return false;
    }
}
void setPresetCamera(brmi_scene& sc) { V3 eye{0, 0, 0}; double yaw = 0, pitch = 0; presetCameraBase(sc.params.preset, eye, yaw, pitch); setCamera(sc, eye, yaw, pitch, 80.0, 0.1, 1000.0); }

void finishFrame(brmi_scene& sc) {
    brmi_per_frame f{};
    std::memset(&f, 0, sizeof(f));
    f.mainCameraIndex = 0; f.numLights = (uint32_t)sc.lights.size();
    f.screenResX = sc.params.width; f.screenResY = sc.params.height;
    f.lightClusterGridSizeX = 12; f.lightClusterGridSizeY = 12; f.lightClusterGridSizeZ = 24;   // BR/src/Renderer.cpp lightClusterSize
    f.nearClusterCount = 4; f.clusterZSplitDepth = 6.0f;                                            // BR/src/Managers/Singletons/ResourceManager.cpp:73-74
    sc.perFrame.push_back(f);
    sc.stats.meshes = (uint32_t)sc.perMesh.size(); sc.stats.instances = (uint32_t)sc.perMeshInstance.size();
    sc.stats.nodes = (uint32_t)sc.nodes.size(); sc.stats.groups = (uint32_t)sc.groups.size(); sc.stats.segments = (uint32_t)sc.segments.size();
    sc.stats.lights = (uint32_t)sc.lights.size(); sc.stats.materials = (uint32_t)sc.materials.size();
}


// Stand-in OpenPBR lookup tables.  The reference includes them from adobe/openpbr-bsdf (absent
// submodule; BR/src/Render/OpenPBRLookupResources.cpp:34-77), so these are synthetic but physically
// plausible: energy complements derived from the MaterialX GGX directional-albedo fit
// (BR/shaders/Include/PBR.hlsli:8-25) and its cosine-weighted averages.  Real tables drop in unchanged.
double ggxDirAlbedo(double x, double y, double F0, double F90) {
    const double c[9][4] = {{0.1003, 0.9345, 1.0, 1.0}, {-0.6303, -2.323, -1.765, 0.2281}, {9.748, 2.229, 8.263, 15.94}, {-2.038, -3.748, 11.53, -55.83},
                            {29.34, 1.424, 28.96, 13.08}, {-8.245, -0.7684, -7.507, 41.26}, {-26.44, 1.436, -36.11, 54.9}, {19.99, 0.2913, 15.86, 300.2}, {-5.448, 0.6286, 33.37, -285.1}};
    double r[4];
    for (int i = 0; i < 4; i++) r[i] = c[0][i] + c[1][i] * x + c[2][i] * y + c[3][i] * x * y + c[4][i] * x * x + c[5][i] * y * y + c[6][i] * x * x * y + c[7][i] * x * y * y + c[8][i] * x * x * y * y;
    double A = std::min(1.0, std::max(0.0, r[0] / r[2])), B = std::min(1.0, std::max(0.0, r[1] / r[3]));
    return F0 * A + F90 * B;
}
void buildLuts(brmi_scene& sc) {
    auto q = [](double v) { return (uint16_t)std::lround(std::min(1.0, std::max(0.0, v)) * 65535.0); };
    const int N = 32;
    sc.lutOdE.resize(N * N * N); sc.lutOdAvg.resize(N * N); sc.lutImE.resize(N * N); sc.lutImAvg.resize(N); sc.lutLtc.resize(N * N * 4);
    auto iorOf = [&](int i) { if (i >= 16) return 1.0 + (i - 16) / 15.0 * 1.5; double fr = (15 - i) / 15.0; return 1.0 / (1.0 + fr * 1.5); };
    for (int a = 0; a < N; a++) {
        const double alpha = (a / 31.0) * (a / 31.0);
        double avg = 0, wsum = 0;
        for (int c = 0; c < N; c++) {
            const double mu = c / 31.0;
            const double comp = 1.0 - ggxDirAlbedo(mu, alpha, 1.0, 1.0);
            sc.lutImE[a * N + c] = q(comp);
        }
        for (int k = 0; k < 256; k++) { double mu = (k + 0.5) / 256.0; avg += (1.0 - ggxDirAlbedo(mu, alpha, 1.0, 1.0)) * mu; wsum += mu; }
        sc.lutImAvg[a] = q(avg / wsum);
        for (int i = 0; i < N; i++) {
            const double ior = iorOf(i), f = (ior - 1.0) / (ior + 1.0), F0 = f * f;
            for (int c = 0; c < N; c++) sc.lutOdE[(i * N + a) * N + c] = q(1.0 - ggxDirAlbedo(c / 31.0, alpha, F0, 1.0));
            double av = 0, ws = 0;
            for (int k = 0; k < 256; k++) { double mu = (k + 0.5) / 256.0; av += (1.0 - ggxDirAlbedo(mu, alpha, F0, 1.0)) * mu; ws += mu; }
            sc.lutOdAvg[i * N + a] = q(av / ws);
        }
    }
    for (int r = 0; r < N; r++) for (int c = 0; c < N; c++) {
        const double rough = r / 31.0, mu = c / 31.0;
        float* t = &sc.lutLtc[(r * N + c) * 4];
        t[0] = (float)(1.0 / (0.15 + 0.85 * rough)); t[1] = (float)(0.6 * (1.0 - mu) * (1.0 - 0.5 * rough)); t[2] = (float)(0.04 + 0.5 * rough * (1.0 - mu) * (1.0 - mu)); t[3] = 0.0f;
    }
}

PatchDef planePatch(V3 origin, V3 U, V3 V, uint32_t nu, uint32_t nv, double amp, double freq, uint32_t seed) {
    PatchDef p; p.type = PATCH_PLANE; p.origin = origin; p.axisU = U; p.axisV = V; p.nu0 = nu; p.nv0 = nv; p.noiseAmp = amp; p.noiseFreq = freq; p.noiseSeed = seed; return p;
}
PatchDef cylinderPatch(V3 base, double r, double h, uint32_t nu, uint32_t nv, double amp, double freq, uint32_t seed) {
    PatchDef p; p.type = PATCH_CYLINDER; p.center = base; p.radiusX = r; p.radiusZ = r; p.height = h; p.nu0 = nu; p.nv0 = nv; p.noiseAmp = amp; p.noiseFreq = freq; p.noiseSeed = seed; return p;
}
PatchDef ellipsoidPatch(V3 c, double rx, double ry, double rz, uint32_t nu, uint32_t nv, double amp, double freq, uint32_t seed) {
    PatchDef p; p.type = PATCH_ELLIPSOID; p.center = c; p.radiusX = rx; p.radiusY = ry; p.radiusZ = rz; p.nu0 = nu; p.nv0 = nv; p.noiseAmp = amp; p.noiseFreq = freq; p.noiseSeed = seed; return p;
}
// closed box as 6 inward- or outward-facing plane patches
void boxPatches(std::vector<PatchDef>& out, V3 lo, V3 hi, uint32_t n, double amp, uint32_t seed) {
    V3 d = hi - lo;
    out.push_back(planePatch({lo.x, hi.y, lo.z}, {0, 0, d.z}, {d.x, 0, 0}, n, n, amp, 3, seed + 0));          // top   (+Y)
    out.push_back(planePatch({lo.x, lo.y, lo.z}, {d.x, 0, 0}, {0, 0, d.z}, n, n, amp, 3, seed + 1));          // bottom(-Y)
    out.push_back(planePatch({lo.x, lo.y, hi.z}, {d.x, 0, 0}, {0, d.y, 0}, n, n, amp, 3, seed + 2));          // +Z
    out.push_back(planePatch({hi.x, lo.y, lo.z}, {-d.x, 0, 0}, {0, d.y, 0}, n, n, amp, 3, seed + 3));         // -Z
    out.push_back(planePatch({hi.x, lo.y, hi.z}, {0, 0, -d.z}, {0, d.y, 0}, n, n, amp, 3, seed + 4));         // +X
    out.push_back(planePatch({lo.x, lo.y, lo.z}, {0, 0, d.z}, {0, d.y, 0}, n, n, amp, 3, seed + 5));          // -X
}

uint32_t roundPow2Mult(uint32_t v, uint32_t levels) { uint32_t q = 1u << (levels - 1); return std::max(q, (v + q - 1) / q * q); }

// A skinning instance slot: 64 joint matrices (bone * inverseBind products, what LoadBoneSkinMatrix multiplies out per
// use; skinningCommon.hlsli:23-48).  Joints 0..3 are the ones the generated meshes reference: a bend along +Y.
uint32_t addSkinSlot(brmi_scene& sc, Pcg32& rng, double amount) {
    const uint32_t slot = (uint32_t)(sc.skinningMatrices.size() / (64 * 16));
    for (uint32_t j = 0; j < 64; j++) {
        const double k = (double)(j & 3) / 3.0;
        // stored as the column-vector product; the shader transposes it into the row-vector skin matrix
        M4 rowVec = mul(mul(rotationZ(amount * 0.6 * k + rng.range(-0.02f, 0.02f)), rotationX(amount * 0.25 * k)), translation({0.15 * amount * k, 0.05 * k, 0.0}));
        M4 stored = transpose(rowVec);
        float f[4][4]; store(f, stored);
        sc.skinningMatrices.insert(sc.skinningMatrices.end(), &f[0][0], &f[0][0] + 16);
    }
    return slot;
}

// ---- presets ---------------------------------------------------------------------------------
void presetTiny(brmi_scene& sc, Pcg32& rng) {
    addMaterials(sc, rng, 4);
    const uint32_t levels = sc.params.lodLevels ? sc.params.lodLevels : 1;
    std::vector<MeshDef> meshes(3);
    meshes[0].patches.push_back(planePatch({-2, 0, -2}, {0, 0, 4}, {4, 0, 0}, roundPow2Mult(2, levels), roundPow2Mult(2, levels), 0.15, 3, 11)); meshes[0].material = 0; meshes[0].lodLevels = levels;
    meshes[1].patches.push_back(ellipsoidPatch({0, 0, 0}, 0.5, 0.5, 0.5, roundPow2Mult(2, levels), roundPow2Mult(1, levels), 0.05, 3, 12)); meshes[1].material = 1; meshes[1].lodLevels = levels;
    meshes[2].patches.push_back(cylinderPatch({0, 0, 0}, 0.25, 1.5, roundPow2Mult(1, levels), roundPow2Mult(2, levels), 0.0, 3, 13)); meshes[2].material = 3; meshes[2].lodLevels = levels;
    const bool skin = sc.params.skinnedFraction1024 != 0;
    if (skin) { meshes.push_back(meshes[1]); meshes.back().skinned = true; meshes.push_back(meshes[2]); meshes.back().skinned = true; }   // meshes 3, 4
    for (size_t i = 0; i < meshes.size(); i++) buildMesh(sc, meshes[i], (uint32_t)i);
    addInstance(sc, {0, identity()});
    addInstance(sc, {1, translation({0.3, 0.6, -0.4})});
    addInstance(sc, {skin ? 3u : 1u, mul(scaling(0.6), translation({-1.0, 0.5, 0.5})), false, skin ? addSkinSlot(sc, rng, 1.0) : 0xFFFFFFFFu});
    addInstance(sc, {2, translation({1.0, 0.0, -1.0})});
    addInstance(sc, {skin ? 4u : 2u, mul(rotationZ(0.3), translation({-0.8, 0.0, -1.2})), false, skin ? addSkinSlot(sc, rng, 1.6) : 0xFFFFFFFFu});
    addInstance(sc, {1, translation({0.0, 0.5, 30.0})});   // behind the camera: frustum-culled
    setPresetCamera(sc);
    if (sc.params.withDirectionalLight) addLight(sc, BRMI_LIGHT_DIRECTIONAL, {0, 0, 0}, {1, 1, 1}, 10.0f, {1, 0, 0}, {0, -6, -1});
    for (uint32_t i = 0; i < sc.params.numPointLights; i++)
        addLight(sc, BRMI_LIGHT_POINT, {rng.range(-2, 2), rng.range(0.2f, 1.5f), rng.range(-2, 2)}, {rng.uniform(), rng.uniform(), rng.uniform()}, 3.0f, {0, 0, 1}, {0, 0, 0});
}

void presetSponza(brmi_scene& sc, Pcg32& rng) {
    // atrium 40 (z) x 14 (x) x 10 (y); ~2048 LOD0 meshlets at sizeScale 1
    addMaterials(sc, rng, 25);
    const uint32_t levels = sc.params.lodLevels ? sc.params.lodLevels : 1;
    const double s = std::sqrt(std::max(0.001f, sc.params.sizeScale));
    auto dim = [&](double v) { return roundPow2Mult((uint32_t)std::max(1.0, std::round(v * s)), levels); };
    std::vector<MeshDef> meshes;
    auto addMesh = [&](std::vector<PatchDef> p, uint32_t mat) { MeshDef m; m.patches = std::move(p); m.material = mat; m.lodLevels = levels; meshes.push_back(std::move(m)); return (uint32_t)meshes.size() - 1; };
    // floor faces +Y : U = +z, V = +x  => U x V = z x x = +y
    uint32_t floor = addMesh({planePatch({-7, 0, -20}, {0, 0, 40}, {14, 0, 0}, dim(32), dim(16), 0.03, 24, 101)}, 0);
    // ceiling faces -Y : U = +x, V = +z => x x z = -y
    uint32_t ceil_ = addMesh({planePatch({-7, 10, -20}, {14, 0, 0}, {0, 0, 40}, dim(16), dim(16), 0.10, 10, 102)}, 1);
    // left wall (x=-7) faces +X : U=+y? need U x V = +x : y x z = +x
    uint32_t wallL = addMesh({planePatch({-7, 0, -20}, {0, 10, 0}, {0, 0, 40}, dim(8), dim(32), 0.08, 16, 103)}, 2);
    // right wall (x=+7) faces -X : z x y = -x
    uint32_t wallR = addMesh({planePatch({7, 0, -20}, {0, 0, 40}, {0, 10, 0}, dim(32), dim(8), 0.08, 16, 104)}, 4);
    // far wall (z=-20) faces +Z : x x y = +z
    uint32_t wallF = addMesh({planePatch({-7, 0, -20}, {14, 0, 0}, {0, 10, 0}, dim(8), dim(8), 0.12, 8, 105)}, 5);
    // near wall (z=+20) faces -Z : y x x = -z
    uint32_t wallN = addMesh({planePatch({-7, 0, 20}, {0, 10, 0}, {14, 0, 0}, dim(8), dim(8), 0.12, 8, 106)}, 6);
    uint32_t column = addMesh({cylinderPatch({0, 0, 0}, 0.45, 8.0, dim(4), dim(8), 0.04, 6, 107)}, 8);
    std::vector<PatchDef> bp; boxPatches(bp, {-0.5, 0, -0.5}, {0.5, 1, 0.5}, dim(1), 0.01, 300);
    uint32_t box = addMesh(bp, 9);
    uint32_t blob = addMesh({ellipsoidPatch({0, 0, 0}, 0.6, 0.6, 0.6, dim(4), dim(2), 0.08, 3, 108)}, 12);
    for (size_t i = 0; i < meshes.size(); i++) buildMesh(sc, meshes[i], (uint32_t)i);
    addInstance(sc, {floor, identity()}); addInstance(sc, {ceil_, identity()}); addInstance(sc, {wallL, identity()});
    addInstance(sc, {wallR, identity()}); addInstance(sc, {wallF, identity()}); addInstance(sc, {wallN, identity()});
    for (int i = 0; i < 8; i++) { double z = -17.5 + 5.0 * i; addInstance(sc, {column, translation({-4.5, 0, z})}); addInstance(sc, {column, translation({4.5, 0, z})}); }
    for (int i = 0; i < 10; i++) {
        double sc1 = rng.range(0.6f, 1.6f);
        addInstance(sc, {box, mul(mul(scaling(sc1), rotationY(rng.range(0, 6.28f))), translation({rng.range(-3.5f, 3.5f), 0, rng.range(-18, 12)}))});
    }
    for (int i = 0; i < 6; i++) addInstance(sc, {blob, mul(scaling(rng.range(0.7f, 1.5f)), translation({rng.range(-3, 3), rng.range(1.0f, 5.0f), rng.range(-16, 8)}))});
    setPresetCamera(sc);
    if (sc.params.withDirectionalLight) addLight(sc, BRMI_LIGHT_DIRECTIONAL, {0, 0, 0}, {1, 1, 1}, 10.0f, {1, 0, 0}, {0, -6, -1});
    for (uint32_t i = 0; i < sc.params.numPointLights; i++)
        addLight(sc, BRMI_LIGHT_POINT, {rng.range(-6.5f, 6.5f), rng.range(0.3f, 9.5f), rng.range(-19.5f, 19.5f)}, {rng.uniform(), rng.uniform(), rng.uniform()}, 3.0f, {0, 0, 1}, {0, 0, 0});
}

void presetStreet(brmi_scene& sc, Pcg32& rng, double triBudget, uint32_t nMeshes, uint32_t nInstances, uint32_t defaultLevels, bool foliage) {
    addMaterials(sc, rng, 64);
    const uint32_t maxLevels = sc.params.lodLevels ? sc.params.lodLevels : defaultLevels;
    const double budgetMeshlets = triBudget * sc.params.sizeScale / 128.0;
    std::vector<MeshDef> meshes;
    auto lv = [&](uint32_t n0) { uint32_t l = 1; while (l < maxLevels && (n0 >> l) >= 1 && ((n0 >> l) << l) == n0) l++; return l; };
    // big statics: ground + two facades (~13 % of the budget at sizeScale 1)
    const double L = 120.0, Wd = 16.0, Hh = 24.0;
    // params.uniqueTriangleBudget: `triBudget` counts the triangles of the MESHES ("~3.0 M tris, ~2,000 instances of ~150 meshes" --
    // 150 meshes of 20 k triangles, each drawn a dozen times; only then can a frame test the 60-80 k meshlets row a-3 speaks of), and every one
    // of the nInstances is placed.  Statics and props get twice the tessellation per dimension of the instanced-budget scene: 4.4 x its 0.67 M
    // unique triangles.  0 (rounds 1-2, the golden fixtures): the budget counts instanced triangles and caps the instance count.
    const bool uniqueBudget = sc.params.uniqueTriangleBudget != 0u;
    const double dimScale = std::sqrt(budgetMeshlets / 23437.5) * (uniqueBudget ? 2.0 : 1.0);
    uint32_t gq = roundPow2Mult((uint32_t)std::max(1.0, std::round(16.0 * dimScale)), maxLevels);
    { MeshDef m; m.patches.push_back(planePatch({-Wd, 0, -L}, {0, 0, 2 * L}, {2 * Wd, 0, 0}, gq * 4, gq, 0.05, 40, 201)); m.material = 0; m.lodLevels = lv(gq); m.reliefScale = 0.15; meshes.push_back(m); }
    uint32_t fq = gq;
    // Facades.  Instanced budget: two 240 m walls of their own.  Unique budget: a street front is a row of houses built from the same parts -- two
    // 30 m facade modules (the second turned round serves the other side of the street), eight of them per side, each tessellated twice as
    // finely per metre as the single wall could afford: 5 cm triangles where the wall had 10 x 23 cm ones.
    const uint32_t kModules = 8;
    if (!uniqueBudget) {
    { MeshDef m; m.patches.push_back(planePatch({-Wd, 0, -L}, {0, Hh, 0}, {0, 0, 2 * L}, fq, fq * 4, 0.35, 30, 202)); m.material = 1; m.lodLevels = lv(fq); meshes.push_back(m); }
    { MeshDef m; m.patches.push_back(planePatch({Wd, 0, -L}, {0, 0, 2 * L}, {0, Hh, 0}, fq * 4, fq, 0.35, 30, 203)); m.material = 2; m.lodLevels = lv(fq); meshes.push_back(m); }
    } else {
        for (uint32_t k = 0; k < 2u; k++) { MeshDef m; m.patches.push_back(planePatch({-Wd, 0, 0}, {0, Hh, 0}, {0, 0, 2 * L / kModules}, fq * 2, fq * 2, 0.35, 4, 202 + k)); m.material = 1 + k; m.lodLevels = lv(fq * 2); meshes.push_back(m); }
    }
    const uint32_t nStatics = (uint32_t)meshes.size();
    // props: sizes drawn from a skewed distribution.  The instance count is capped, so a budget beyond sizeScale 4 goes into the props'
    // tessellation (a power of two per dimension: the LOD levels halve it): the dense workloads put their triangles where the camera looks
    uint32_t propTess = 1; while (sc.params.sizeScale >= 4.0f * (float)(propTess * propTess)) propTess *= 2u;
    if (uniqueBudget) propTess *= 2u;
    const uint32_t nProps = std::max(1u, nMeshes - nStatics);
    std::vector<uint32_t> propMeshlets(nProps);
    for (uint32_t i = 0; i < nProps; i++) {
        float u = rng.uniform();
        uint32_t a = (u < 0.55f) ? 1u : (u < 0.85f ? 2u : (u < 0.97f ? 4u : 8u));   // meshlets per dim (nv); nu = 2a
        if (foliage && (i % 3) == 0) a = 1;
        if (maxLevels == 1) a = std::min(a, 4u);
        a *= propTess;
        MeshDef m;
        uint32_t kind = foliage && (i % 3) == 0 ? 3u : (i % 3);
        uint32_t seed = 400 + i;
        if (kind == 0) m.patches.push_back(ellipsoidPatch({0, 0, 0}, rng.range(0.4f, 1.2f), rng.range(0.4f, 1.6f), rng.range(0.4f, 1.2f), 2 * a, a, rng.range(0.02f, 0.2f), 3, seed));
        else if (kind == 1) m.patches.push_back(cylinderPatch({0, 0, 0}, rng.range(0.15f, 0.6f), rng.range(1.0f, 6.0f), a, 2 * a, rng.range(0.0f, 0.1f), 5, seed));
        else if (kind == 2) { boxPatches(m.patches, {-0.7, 0, -0.5}, {0.7, rng.range(0.5f, 2.5f), 0.5}, std::max(1u, a / 2), 0.02, seed); }
        else { // foliage card: two crossed double-sided-ish quads (two opposite-facing planes each)
            double h = rng.range(0.8f, 2.5f), w = rng.range(0.5f, 1.5f);
            m.patches.push_back(planePatch({-w, 0, 0}, {2 * w, 0, 0}, {0, h, 0}, a, a, 0.15, 4, seed));
            m.patches.push_back(planePatch({w, 0, 0}, {-2 * w, 0, 0}, {0, h, 0}, a, a, 0.15, 4, seed + 1000));
            m.patches.push_back(planePatch({0, 0, -w}, {0, 0, 2 * w}, {0, h, 0}, a, a, 0.15, 4, seed + 2000));
            m.patches.push_back(planePatch({0, 0, w}, {0, 0, -2 * w}, {0, h, 0}, a, a, 0.15, 4, seed + 3000));
        }
        uint32_t minDim = 0xFFFFFFFFu; for (auto& p : m.patches) minDim = std::min(minDim, std::min(p.nu0, p.nv0));
        m.lodLevels = lv(minDim);
        m.material = 3 + rng.below(60);
        uint32_t cnt = 0; for (auto& p : m.patches) cnt += p.nu0 * p.nv0;
        propMeshlets[i] = cnt;
        m.skinned = ((i * 2654435761u) >> 22) < sc.params.skinnedFraction1024;     // hash of the prop index: does not disturb the scene's random stream
        meshes.push_back(m);
    }
    for (size_t i = 0; i < meshes.size(); i++) buildMesh(sc, meshes[i], (uint32_t)i);
    if (!uniqueBudget) for (uint32_t i = 0; i < nStatics; i++) addInstance(sc, {i, identity()});
    else {
        addInstance(sc, {0, identity()});
        for (uint32_t k = 0; k < kModules; k++) {
            const double z0 = -L + 2 * L / kModules * k;
            addInstance(sc, {1 + (k & 1u), translation({0, 0, z0})});                                                   // x = -Wd, facing +x
            addInstance(sc, {2 - (k & 1u), mul(rotationY(M_PI), translation({0, 0, z0 + 2 * L / kModules}))});          // turned round: x = +Wd, facing -x
        }
    }
    // instances: fill the remaining budget
    double remaining = budgetMeshlets - (double)sc.stats.instancedTriangles / 128.0;
    uint32_t made = 0;
    Pcg32 skinRng(sc.params.seed * 977u + 5u, 77u);
    while (made < nInstances && (remaining > 0 || uniqueBudget)) {
        uint32_t pi = rng.below(nProps);
        double scl = rng.range(0.5f, 1.8f);
        // 70 % on the street band, 30 % anywhere incl. behind the camera / behind facades
        V3 pos;
        if (rng.uniform() < 0.7f) pos = {rng.range((float)-Wd + 1, (float)Wd - 1), 0, rng.range((float)-L + 2, 20.0f)};
        else pos = {rng.range((float)-Wd * 2.5f, (float)Wd * 2.5f), 0, rng.range((float)-L, (float)L)};
        if (foliage) pos.y = rng.range(0.0f, 3.0f);
        // a street has a carriageway: nothing stands within 3.5 m of the camera's path (x = 0.8, z from 34 down to 4), or the frame is one prop's back
        if (uniqueBudget && std::fabs(pos.x - 0.8) < 3.5 && pos.z > 4.0) continue;
        const M4 xf = mul(mul(scaling(scl), rotationY(rng.range(0, 6.2831f))), translation(pos));
        addInstance(sc, {nStatics + pi, xf, false, meshes[nStatics + pi].skinned ? addSkinSlot(sc, skinRng, skinRng.range(0.3f, 1.5f)) : 0xFFFFFFFFu});
        remaining -= propMeshlets[pi];
        made++;
    }
    setPresetCamera(sc);
    if (sc.params.withDirectionalLight) addLight(sc, BRMI_LIGHT_DIRECTIONAL, {0, 0, 0}, {1, 1, 1}, 10.0f, {1, 0, 0}, {0, -6, -1});
    for (uint32_t i = 0; i < sc.params.numPointLights; i++)
        addLight(sc, BRMI_LIGHT_POINT, {rng.range((float)-Wd + 0.5f, (float)Wd - 0.5f), rng.range(0.3f, 6.0f), rng.range(-90.0f, 30.0f)}, {rng.uniform(), rng.uniform(), rng.uniform()}, 3.0f, {0, 0, 1}, {0, 0, 0});
}

void presetZorah(brmi_scene& sc, Pcg32& rng) {
    addMaterials(sc, rng, 16);
    const uint32_t levels = sc.params.lodLevels ? sc.params.lodLevels : 6;
    // one detailed mesh (~100k tris at sizeScale 1: 32x24 = 768 meshlets) instanced on a huge grid
    MeshDef m; uint32_t a = roundPow2Mult(16, levels);
    m.patches.push_back(ellipsoidPatch({0, 1.0, 0}, 1.0, 1.0, 1.0, 2 * a, a, 0.25, 6, 900));
    m.patches.push_back(cylinderPatch({0, -1.0, 0}, 0.6, 1.2, a, a, 0.05, 4, 901));
    m.lodLevels = levels; m.material = 1;
    buildMesh(sc, m, 0);
    MeshDef g; g.patches.push_back(planePatch({-2000, -1.0, -4000}, {0, 0, 4200}, {4000, 0, 0}, roundPow2Mult(64, levels), roundPow2Mult(64, levels), 1.5, 200, 902)); g.lodLevels = levels; g.material = 0;
    buildMesh(sc, g, 1);
    addInstance(sc, {1, identity()});
    const uint32_t n = (uint32_t)std::max(1.0, 100000.0 * sc.params.sizeScale);
    const uint32_t side = (uint32_t)std::ceil(std::sqrt((double)n));
    for (uint32_t i = 0; i < n; i++) {
        double x = ((double)(i % side) - side / 2.0) * 3.2 + rng.range(-0.8f, 0.8f), z = -((double)(i / side)) * 3.2 + 10.0 + rng.range(-0.8f, 0.8f);
        addInstance(sc, {0, mul(mul(scaling(rng.range(0.7f, 1.3f)), rotationY(rng.range(0, 6.2831f))), translation({x, 0.0, z}))});
    }
    setPresetCamera(sc);
    if (sc.params.withDirectionalLight) addLight(sc, BRMI_LIGHT_DIRECTIONAL, {0, 0, 0}, {1, 1, 1}, 10.0f, {1, 0, 0}, {0, -6, -1});
    for (uint32_t i = 0; i < sc.params.numPointLights; i++)
        addLight(sc, BRMI_LIGHT_POINT, {rng.range(-40, 40), rng.range(0.5f, 4.0f), rng.range(-120, 15)}, {rng.uniform(), rng.uniform(), rng.uniform()}, 3.0f, {0, 0, 1}, {0, 0, 0});
}

}  // namespace

extern "C" {

static brmi_scene* createScene(const brmi_scene_params* params, const char* cacheDir, brmi_dag_build_fn build = nullptr, brmi_dag_release_fn release = nullptr, void* user = nullptr) {
    if (!params || params->width == 0 || params->height == 0) return nullptr;
    brmi_scene* sc = new brmi_scene();
    sc->params = *params;
    if (cacheDir) sc->cacheDir = cacheDir;
    if (sc->params.sizeScale <= 0.0f) sc->params.sizeScale = 1.0f;
    if (!(sc->params.detail > 1.0f)) sc->params.detail = 1.0f;
    if (sc->params.lodBuilder == BRMI_LOD_BUILDER_OWN) { sc->dagBuild = brmi_lod_build; sc->dagRelease = brmi_lod_release; }
    else if (sc->params.lodBuilder == BRMI_LOD_BUILDER_EXTERNAL) { sc->dagBuild = build; sc->dagRelease = release; sc->dagUser = user; }
    if (sc->params.lodBuilder > BRMI_LOD_BUILDER_OWN || (sc->params.lodBuilder == BRMI_LOD_BUILDER_EXTERNAL && !build && !cacheDir)) { delete sc; return nullptr; }
    for (int k = 0; k < 3; k++) { sc->stats.sceneMin[k] = 1e30f; sc->stats.sceneMax[k] = -1e30f; }
    Pcg32 rng(0xB451C0DEull + params->seed, 54u + params->preset);
    switch (params->preset) {
        case BRMI_PRESET_TINY: presetTiny(*sc, rng); break;
        case BRMI_PRESET_SPONZA: presetSponza(*sc, rng); break;
        case BRMI_PRESET_BISTRO: presetStreet(*sc, rng, 3.0e6, 150, 2000, 5, false); break;
        case BRMI_PRESET_SAN_MIGUEL: presetStreet(*sc, rng, 10.0e6, 220, 9000, 5, true); break;
        case BRMI_PRESET_ZORAH: presetZorah(*sc, rng); break;
        default: delete sc; return nullptr;
    }
    if (sc->failed) { delete sc; return nullptr; }
    buildLuts(*sc);
    finishFrame(*sc);
    return sc;
}
brmi_scene* brmi_scene_create(const brmi_scene_params* params) { return createScene(params, nullptr); }

int brmi_scene_camera_at(const brmi_scene_params* params, double step, double prevStep, brmi_camera* camera, brmi_culling_camera* cullingCamera) {
    if (!params || !camera || !cullingCamera || params->width == 0 || params->height == 0 || !(step >= 0.0) || !(prevStep >= 0.0)) return -1;
    V3 eye; double yaw, pitch;
    if (!presetCameraBase(params->preset, eye, yaw, pitch)) return -1;
    makeCamera(params->width, params->height, eye, yaw, pitch, 80.0, 0.1, 1000.0, step, prevStep, *camera, *cullingCamera);
    return 0;
}

// the caller's materials, textures and samplers where addMaterials puts the procedural ones; false on input the tables cannot hold
static bool addUserMaterials(brmi_scene& sc, const brmi_material_inputs& in) {
    if (in.structSize != sizeof(brmi_material_inputs) || !in.materials || in.materialCount == 0 || (in.textureCount && !in.textures) || (in.samplerCount && !in.samplers) ||
        (in.openpbrCount && !in.openpbr)) return false;
    sc.srgbToLinear.resize(256);
    for (int c = 0; c < 256; c++) { const double x = c / 255.0; sc.srgbToLinear[c] = (float)(x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4)); }
    for (uint32_t t = 0; t < in.textureCount; t++) {
        brmi_texture_desc d = in.textures[t];
        if (!d.texels || d.width == 0 || d.height == 0 || d.width > 16384u || d.height > 16384u || d.mipCount == 0 || d.mipCount > BRMI_TEXTURE_MAX_MIPS ||
            (d.format != BRMI_TEXTURE_FORMAT_RGBA8_UNORM && d.format != BRMI_TEXTURE_FORMAT_RGBA8_UNORM_SRGB)) return false;
        uint32_t full = 0; for (uint32_t m = std::max(d.width, d.height); m; m >>= 1) full++;
        if (d.mipCount > full) return false;
        const uint8_t* level0 = d.texels;
        d.texels = reinterpret_cast<const uint8_t*>((uintptr_t)sc.texels.size());
        uint64_t at = 0;
        for (uint32_t l = 0; l < d.mipCount; l++) { d.mipOffset[l] = (uint32_t)at; at += (uint64_t)std::max(1u, d.width >> l) * std::max(1u, d.height >> l); }
        for (uint32_t l = d.mipCount; l < BRMI_TEXTURE_MAX_MIPS; l++) d.mipOffset[l] = 0;
        if (at > 0xFFFFFFFFull) return false;
        const size_t base = sc.texels.size();
        sc.texels.resize(base + (size_t)at * 4, 0);                                 // the whole chain reserved; levels 1.. are for brmi_texmips_build[_alpha]
        std::memcpy(sc.texels.data() + base, level0, (size_t)d.width * d.height * 4);
        sc.textureDescs.push_back(d);
    }
    sc.samplerDescs.assign(in.samplers, in.samplers + in.samplerCount);
    sc.materials.assign(in.materials, in.materials + in.materialCount);
    uint32_t sets = 1;
    for (brmi_material_info& m : sc.materials) {
        const uint32_t named[8] = {m.baseColorUvSetIndex, m.normalUvSetIndex, m.metallicUvSetIndex, m.roughnessUvSetIndex, m.emissiveUvSetIndex, m.aoUvSetIndex, m.heightUvSetIndex, m.opacityUvSetIndex};
        for (uint32_t k : named) if (k < 2u) sets = std::max(sets, k + 1u);
    }
    sc.userUvSets = sets;
    // a slot a material's flags switch on must name a texture and a sampler of the tables (the kernels read a dangling index as "not bound": here it is a mistake of the caller's)
    for (const brmi_material_info& m : sc.materials) {
        const struct { uint32_t flag, texture, sampler; } slots[8] = {
            {BRMI_MATERIAL_BASE_COLOR_TEXTURE, m.baseColorTextureIndex, m.baseColorSamplerIndex}, {BRMI_MATERIAL_NORMAL_MAP, m.normalTextureIndex, m.normalSamplerIndex},
            {BRMI_MATERIAL_METALLIC_TEXTURE, m.metallicTextureIndex, m.metallicSamplerIndex}, {BRMI_MATERIAL_ROUGHNESS_TEXTURE, m.roughnessTextureIndex, m.roughnessSamplerIndex},
            {BRMI_MATERIAL_EMISSIVE_TEXTURE, m.emissiveTextureIndex, m.emissiveSamplerIndex}, {BRMI_MATERIAL_AO_TEXTURE, m.aoMapIndex, m.aoSamplerIndex},
            {BRMI_MATERIAL_PARALLAX, m.heightMapIndex, m.heightSamplerIndex}, {BRMI_MATERIAL_OPACITY_TEXTURE, m.opacityTextureIndex, m.opacitySamplerIndex}};
        for (const auto& sl : slots) if ((m.materialFlags & sl.flag) && (sl.texture >= in.textureCount || sl.sampler >= in.samplerCount)) return false;
    }
    if (in.openpbrCount) sc.openpbr.assign(in.openpbr, in.openpbr + in.openpbrCount);
    else for (uint32_t i = 0; i < in.materialCount; i++) {      // the base layer of the material's own factors, no coat, no fuzz
        brmi_material_info& m = sc.materials[i];
        m.openPBRMaterialDataIndex = i;
        brmi_openpbr_material_info o{};
        std::memset(&o, 0, sizeof(o));
        o.baseWeight = 1.0f; o.baseColor[0] = m.baseColorFactor[0]; o.baseColor[1] = m.baseColorFactor[1]; o.baseColor[2] = m.baseColorFactor[2];
        o.baseMetalness = m.metallicFactor; o.specularWeight = 1.0f; o.specularColor[0] = o.specularColor[1] = o.specularColor[2] = 1.0f;
        o.specularRoughness = m.roughnessFactor; o.specularIor = 1.5f; o.specularAnisotropyRotationCosSin[0] = 1.0f;
        o.coatColor[0] = o.coatColor[1] = o.coatColor[2] = 1.0f; o.coatIor = 1.6f; o.coatDarkening = 1.0f; o.coatAnisotropyRotationCosSin[0] = 1.0f;
        o.fuzzColor[0] = o.fuzzColor[1] = o.fuzzColor[2] = 1.0f; o.fuzzRoughness = 0.5f;
        o.transmissionColor[0] = o.transmissionColor[1] = o.transmissionColor[2] = 1.0f; o.thinFilmIor = 1.4f; o.geometryOpacity = 1.0f;
        for (int k = 0; k < 12; k++) o.textureBindings[k] = 0xFFFFFFFFu;
        for (int k = 0; k < 4; k++) { o.textureBindings[12 + k] = (uint32_t)k; o.textureBindings[19 + k] = (uint32_t)k; }
        sc.openpbr.push_back(o);
    }
    for (const brmi_material_info& m : sc.materials) if (m.openPBRMaterialDataIndex >= sc.openpbr.size()) return false;
    return true;
}
static brmi_scene* createFromMeshes(const brmi_scene_params* params, const brmi_mesh_input* meshes, uint32_t meshCount, const brmi_instance_input* instances, uint32_t instanceCount,
                                    const brmi_view_input* view, const brmi_material_inputs* mats, brmi_dag_build_fn build, brmi_dag_release_fn release, void* user) {
    if (!params || params->width == 0 || params->height == 0 || !meshes || meshCount == 0 || !instances || instanceCount == 0 || !view) return nullptr;
    if (!(view->zNear > 0.0f) || !(view->zFar > view->zNear) || !(view->fovYDegrees > 0.0f) || !(view->fovYDegrees < 180.0f)) return nullptr;
    uint32_t materialCount = 1;
    for (uint32_t m = 0; m < meshCount; m++) {
        const brmi_mesh_input& u = meshes[m];
        if (!u.positions || !u.indices || u.vertexCount == 0 || u.indexCount < 3 || u.indexCount % 3 != 0 || u.vertexCount > 0x7FFFFFFFull || u.material > 4095u) return nullptr;
        for (size_t i = 0; i < u.indexCount; i++) if (u.indices[i] >= u.vertexCount) return nullptr;
        for (size_t i = 0; i < u.vertexCount * 3; i++) if (!std::isfinite(u.positions[i])) return nullptr;
        materialCount = std::max(materialCount, u.material + 1u);
    }
    for (uint32_t i = 0; i < instanceCount; i++) {
        if (instances[i].mesh >= meshCount) return nullptr;
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) if (!std::isfinite(instances[i].model[r][c])) return nullptr;
    }
    brmi_scene* sc = new brmi_scene();
    sc->params = *params;
    if (sc->params.sizeScale <= 0.0f) sc->params.sizeScale = 1.0f;
    sc->params.detail = 1.0f;
    if (sc->params.lodBuilder == BRMI_LOD_BUILDER_EXTERNAL && build) { sc->dagBuild = build; sc->dagRelease = release; sc->dagUser = user; }
    else { sc->params.lodBuilder = BRMI_LOD_BUILDER_OWN; sc->dagBuild = brmi_lod_build; sc->dagRelease = brmi_lod_release; }      // (the quadtree builder only knows the procedural patches)
    for (int k = 0; k < 3; k++) { sc->stats.sceneMin[k] = 1e30f; sc->stats.sceneMax[k] = -1e30f; }
    Pcg32 rng(0xB451C0DEull + params->seed, 54u + 77u);
    if (!mats) addMaterials(*sc, rng, materialCount);
    else {
        // a mesh may only name a material of the caller's table; the pages carry a UV stream whenever a texture is there to be sampled
        if (materialCount > mats->materialCount || !addUserMaterials(*sc, *mats)) { delete sc; return nullptr; }
        sc->params.materialFeatures = (sc->params.materialFeatures & 32u) | (mats->textureCount ? 8u : 0u);
    }
    for (uint32_t m = 0; m < meshCount && !sc->failed; m++) {
        MeshDef def; def.user = &meshes[m]; def.material = meshes[m].material; def.lodLevels = sc->params.lodLevels ? sc->params.lodLevels : 1;
        if (mats && mats->uvs1) def.userUvs1 = mats->uvs1[m];
        buildMesh(*sc, def, m);
    }
    if (sc->failed) { delete sc; return nullptr; }
    for (uint32_t i = 0; i < instanceCount; i++) {
        M4 model{};
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) model.m[r][c] = instances[i].model[r][c];
        addInstance(*sc, {instances[i].mesh, model, instances[i].reverseWinding != 0});
    }
    setCamera(*sc, V3{view->eye[0], view->eye[1], view->eye[2]}, view->yaw, view->pitch, view->fovYDegrees, view->zNear, view->zFar);
    const V3 lo{sc->stats.sceneMin[0], sc->stats.sceneMin[1], sc->stats.sceneMin[2]}, hi{sc->stats.sceneMax[0], sc->stats.sceneMax[1], sc->stats.sceneMax[2]};
    const double extent = std::max(1e-3, std::max(hi.x - lo.x, std::max(hi.y - lo.y, hi.z - lo.z)));
    if (sc->params.withDirectionalLight) addLight(*sc, BRMI_LIGHT_DIRECTIONAL, {0, 0, 0}, {1, 1, 1}, 10.0f, {1, 0, 0}, {-0.3, -1.0, -0.4});
    for (uint32_t i = 0; i < sc->params.numPointLights; i++)
        addLight(*sc, BRMI_LIGHT_POINT, {rng.range((float)lo.x, (float)hi.x), rng.range((float)lo.y, (float)hi.y), rng.range((float)lo.z, (float)hi.z)}, {rng.uniform(), rng.uniform(), rng.uniform()},
                 (float)(3.0 * extent * extent / 16.0), {0, 0, 1}, {0, 0, 0});
    buildLuts(*sc);
    finishFrame(*sc);
    return sc;
}
brmi_scene* brmi_scene_create_from_meshes(const brmi_scene_params* params, const brmi_mesh_input* meshes, uint32_t meshCount, const brmi_instance_input* instances, uint32_t instanceCount,
                                          const brmi_view_input* view, brmi_dag_build_fn build, brmi_dag_release_fn release, void* user) {
    return createFromMeshes(params, meshes, meshCount, instances, instanceCount, view, nullptr, build, release, user);
}
brmi_scene* brmi_scene_create_from_meshes_with_materials(const brmi_scene_params* params, const brmi_mesh_input* meshes, uint32_t meshCount, const brmi_instance_input* instances,
                                                         uint32_t instanceCount, const brmi_view_input* view, const brmi_material_inputs* materials,
                                                         brmi_dag_build_fn build, brmi_dag_release_fn release, void* user) {
    if (!materials) return nullptr;
    return createFromMeshes(params, meshes, meshCount, instances, instanceCount, view, materials, build, release, user);
}
brmi_scene* brmi_scene_create_with_dag_builder(const brmi_scene_params* params, brmi_dag_build_fn build, brmi_dag_release_fn release, void* user) {
    if (!params || params->lodBuilder != BRMI_LOD_BUILDER_EXTERNAL || !build) return nullptr;
    return createScene(params, nullptr, build, release, user);
}

void brmi_scene_destroy(brmi_scene* scene) { delete scene; }

int brmi_scene_export_cache(const brmi_scene* s, const char* directory) {
    if (!s || !directory || s->meshCache.size() != s->meshMetadata.size()) return -1;
    for (uint32_t m = 0; m < (uint32_t)s->meshMetadata.size(); m++) if (!saveMeshCache(collectMeshCache(*s, m), directory, m)) return -2;
    return (int)s->meshMetadata.size();
}

brmi_scene* brmi_scene_create_from_cache(const brmi_scene_params* params, const char* directory) {
    if (!directory || !*directory) return nullptr;
    return createScene(params, directory);
}

int brmi_scene_array(const brmi_scene* s, uint32_t id, const void** ptr, uint64_t* bytes, uint32_t* count) {
    if (!s || !ptr || !bytes || !count) return -1;
#define ARR(vec, elem) do { *ptr = (vec).data(); *bytes = (uint64_t)(vec).size() * sizeof((vec)[0]); *count = (uint32_t)((vec).size() / (elem)); return 0; } while (0)
    switch (id) {
        case BRMI_ARR_PER_OBJECT: ARR(s->perObject, 1);
        case BRMI_ARR_NORMAL_MATRICES: ARR(s->normalMatrices, 16);
        case BRMI_ARR_PER_MESH: ARR(s->perMesh, 1);
        case BRMI_ARR_PER_MESH_INSTANCE: ARR(s->perMeshInstance, 1);
        case BRMI_ARR_CLOD_OFFSETS: ARR(s->clodOffsets, 1);
        case BRMI_ARR_CLOD_MESH_METADATA: ARR(s->meshMetadata, 1);
        case BRMI_ARR_LOD_NODES: ARR(s->nodes, 1);
        case BRMI_ARR_LOD_GROUPS: ARR(s->groups, 1);
        case BRMI_ARR_LOD_SEGMENTS: ARR(s->segments, 1);
        case BRMI_ARR_GROUP_PAGE_MAP: ARR(s->pageMap, 1);
        case BRMI_ARR_MATERIALS: ARR(s->materials, 1);
        case BRMI_ARR_OPENPBR_MATERIALS: ARR(s->openpbr, 1);
        case BRMI_ARR_LIGHTS: ARR(s->lights, 1);
        case BRMI_ARR_ACTIVE_LIGHT_INDICES: ARR(s->activeLights, 1);
        case BRMI_ARR_CAMERAS: ARR(s->cameras, 1);
        case BRMI_ARR_CULLING_CAMERAS: ARR(s->cullingCameras, 1);
        case BRMI_ARR_VIEW_RASTER_INFO: ARR(s->viewRasterInfo, 1);
        case BRMI_ARR_PER_FRAME: ARR(s->perFrame, 1);
        case BRMI_ARR_ACTIVE_DRAWS: ARR(s->activeDraws, 1);
        case BRMI_ARR_SKINNING_MATRICES: ARR(s->skinningMatrices, 16);
        case BRMI_ARR_LUT_OD_ENERGY: ARR(s->lutOdE, 1);
        case BRMI_ARR_LUT_OD_AVG_ENERGY: ARR(s->lutOdAvg, 1);
        case BRMI_ARR_LUT_IM_ENERGY: ARR(s->lutImE, 1);
        case BRMI_ARR_LUT_IM_AVG_ENERGY: ARR(s->lutImAvg, 1);
        case BRMI_ARR_LUT_FUZZ_LTC: ARR(s->lutLtc, 4);
        case BRMI_ARR_TEXTURE_DESCS: ARR(s->textureDescs, 1);
        case BRMI_ARR_TEXELS: ARR(s->texels, 1);
        case BRMI_ARR_SAMPLER_DESCS: ARR(s->samplerDescs, 1);
        case BRMI_ARR_SRGB_TO_LINEAR: ARR(s->srgbToLinear, 1);
        default: return -1;
    }
#undef ARR
}

uint32_t brmi_scene_slab_count(const brmi_scene* s) { return s && !s->slabs.empty() ? (uint32_t)s->slabs.size() - 1 : 0; }
int brmi_scene_slab(const brmi_scene* s, uint32_t i, const void** ptr, uint64_t* bytes) {
    if (!s || i == 0 || i >= s->slabs.size()) return -1;
    *ptr = s->slabs[i].data(); *bytes = s->slabs[i].size(); return 0;
}
void brmi_scene_get_stats(const brmi_scene* s, brmi_scene_stats* out) { if (s && out) *out = s->stats; }

}  // extern "C"
