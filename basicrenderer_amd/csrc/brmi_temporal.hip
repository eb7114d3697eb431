// brmi_temporal.hip -- the temporal resolve for gfx950: the jittered one-sample frame and last frame's resolved image into this frame's.
//
// The reference hands this stage to DLSS / FSR; the arithmetic here is the project's own and lives in brmi_temporal_math.h, shared with the host.
//   * a 256-thread workgroup takes a 16 x 16 block, 2 x 2 tiles of the surfaces' tiled 8x8 layout, a wave per tile: a wave's own pixels load and store as one
//     contiguous run (512 B of colour, 256 B of depth);
//   * the block's 18 x 18 halo of w-space colour (three halves) and depth goes into LDS once: every thread stages its own pixel, 68 threads one rim pixel each.
//     Coordinates are clamped to the frame BEFORE the load, so the rim of the frame repeats its edge and no address lies outside the W x H pixels' own tiles;
//   * LDS is column-major with 24 entries a column, as a tile's lanes are (lane = 8 x + y): the 32 lanes of a half wave read four columns of eight, dword addresses
//     24 x + y -- banks {0, 24, 16, 8} + y, all 32 distinct for ds_read_b32 -- and for the 8 B colour entries 48 x + 2 y (+1), all 64 distinct for ds_read_b64;
//   * the motion word of the closest neighbour and the four history taps are gathers from global memory (neighbouring lanes, neighbouring addresses).
// Wave64, no scratch; 18 x 24 x 12 B = 5184 B of LDS.
#include "brmi_internal.h"
#include "brmi_temporal_math.h"

namespace brmi {

namespace tm = temporal;

struct TemporalArgs { const uint2* hdr; const float* depth; const uint32_t* motion; const uint2* history; uint2* out; uint32_t W, H, tilesX; float blend; };

constexpr uint32_t kHalo = 18u, kHaloStride = 24u;

__global__ void __launch_bounds__(256) k_temporal_resolve(TemporalArgs a) {
    __shared__ uint2 colour[kHalo * kHaloStride];
    __shared__ float depth[kHalo * kHaloStride];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t bx = blockIdx.x * 16u, by = blockIdx.y * 16u;
    const uint32_t lx = (wave & 1u) * 8u + (lane >> 3), ly = (wave >> 1) * 8u + (lane & 7u);      // in the block
    const uint32_t px = bx + lx, py = by + ly;
    const uint32_t maxX = a.W - 1u, maxY = a.H - 1u;
    auto stage = [&](uint32_t hx, uint32_t hy) {      // halo cell (hx, hy) is pixel (bx + hx - 1, by + hy - 1), clamped to the frame
        const uint32_t gx = bx + hx, gy = by + hy;
        const uint32_t x = gx == 0u ? 0u : (gx - 1u > maxX ? maxX : gx - 1u), y = gy == 0u ? 0u : (gy - 1u > maxY ? maxY : gy - 1u);
        const uint32_t i = tiled_index(x, y, a.tilesX);
        const uint2 c = a.hdr[i];
        uint2 w;
        tm::to_w_halves(c.x, c.y, w.x, w.y);
        colour[hx * kHaloStride + hy] = w;
        depth[hx * kHaloStride + hy] = a.depth[i];
    };
    stage(lx + 1u, ly + 1u);
    if (threadIdx.x < 68u) {      // the rim: 18 above, 18 below, 16 left, 16 right
        const uint32_t t = threadIdx.x;
        if (t < 36u) stage(t % 18u, t < 18u ? 0u : 17u);
        else stage(t < 52u ? 0u : 17u, 1u + (t - 36u) % 16u);
    }
    __syncthreads();
    if (px >= a.W || py >= a.H) return;

    tm::Box box{}; float best = 0.0f; uint32_t bestX = 0u, bestY = 0u;
#pragma unroll
    for (uint32_t dy = 0u; dy < 3u; dy++) {
#pragma unroll
        for (uint32_t dx = 0u; dx < 3u; dx++) {
            const uint32_t cell = (lx + dx) * kHaloStride + (ly + dy);
            const uint2 wv = colour[cell];
            const tm::rgb w = tm::unpack_rgb(wv.x, wv.y);
            const float d = depth[cell];
            if (dy == 0u && dx == 0u) { tm::box_start(box, w); best = d; bestX = dx; bestY = dy; }
            else { tm::box_add(box, w); if (tm::closer(d, best)) { best = d; bestX = dx; bestY = dy; } }
        }
    }
    const uint32_t i = tiled_index(px, py, a.tilesX);
    uint2 result = a.hdr[i];      // history absent: the current colour unchanged
    if (a.history) {
        // the closest neighbour's pixel, clamped as it was staged
        const uint32_t gx = px + bestX, gy = py + bestY;
        const uint32_t vx = gx == 0u ? 0u : (gx - 1u > maxX ? maxX : gx - 1u), vy = gy == 0u ? 0u : (gy - 1u > maxY ? maxY : gy - 1u);
        const uint32_t mv = a.motion[tiled_index(vx, vy, a.tilesX)];
        const tm::Tap t = tm::tap_of(px, py, tm::half_value(mv & 0xFFFFu), tm::half_value(mv >> 16), a.W, a.H);
        if (t.inside) {
            const uint2 h00 = a.history[tiled_index(t.x0, t.y0, a.tilesX)], h10 = a.history[tiled_index(t.x1, t.y0, a.tilesX)];
            const uint2 h01 = a.history[tiled_index(t.x0, t.y1, a.tilesX)], h11 = a.history[tiled_index(t.x1, t.y1, a.tilesX)];
            const tm::rgb h = tm::tap_mix(tm::unpack_rgb(h00.x, h00.y), tm::unpack_rgb(h10.x, h10.y), tm::unpack_rgb(h01.x, h01.y), tm::unpack_rgb(h11.x, h11.y), t.fx, t.fy);
            if (tm::finite3(h)) {
                const uint2 cv = colour[(lx + 1u) * kHaloStride + (ly + 1u)];
                tm::resolve_words(h, tm::unpack_rgb(cv.x, cv.y), box, a.blend, result.y >> 16, result.x, result.y);
            }
        }
    }
    a.out[i] = result;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------------------------
uint64_t temporal_image_bytes(uint32_t width, uint32_t height) { return (uint64_t)((width + 7u) / 8u) * ((height + 7u) / 8u) * 64u * 8u; }

hipError_t launch_temporal_surfaces(uint32_t width, uint32_t height, const void* hdr, const void* depth, const void* motion, const void* history, void* out, float blend, hipStream_t s) {
    TemporalArgs a{};
    a.hdr = static_cast<const uint2*>(hdr); a.depth = static_cast<const float*>(depth); a.motion = static_cast<const uint32_t*>(motion);
    a.history = static_cast<const uint2*>(history); a.out = static_cast<uint2*>(out);
    a.W = width; a.H = height; a.tilesX = (width + 7u) / 8u; a.blend = blend;
    hipLaunchKernelGGL(k_temporal_resolve, dim3((width + 15u) / 16u, (height + 15u) / 16u), dim3(256), 0, s, a);
    return hipGetLastError();
}
// reads the image the pass wrote last (none while the history is invalid), writes the other one, and makes that the image the next frame and the display chain read
int launch_temporal_resolve(brmi_pass* p, hipStream_t s) {
    auto& t = p->temporal;
    const void* history = t.valid ? t.b.history[t.last] : nullptr;
    void* out = t.b.history[t.last ^ 1u];
    const hipError_t e = launch_temporal_surfaces(p->cfg.width, p->cfg.height, p->res[BRMI_RES_HDR_COLOR], p->res[BRMI_RES_LINEAR_DEPTH], p->res[BRMI_RES_GBUF_MOTION_VECTORS], history, out, t.b.settings.blend, s);
    if (e != hipSuccess) return fail(p, BRMI_ERR_HIP, "launch k_temporal_resolve: %s", hipGetErrorString(e));
    t.last ^= 1u; t.valid = true;
    return BRMI_OK;
}

}  // namespace brmi
