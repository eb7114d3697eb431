// temporal_main.cpp -- brmi_temporal_math.h on the host, alone: tests/test_temporal_cpu.py builds it with the library's floating-point rules and compares its output
// with tests/temporal_ref.py bit for bit.
//
//   temporal_main IN OUT        IN: u32 W, H, haveHistory; f32 blend; then row-major images: hdr (u64), depth (f32), motion (u32), history (u64, if haveHistory).
//                               OUT: the resolved image (u64, row-major).
//   temporal_main --jitter N P  prints N lines "jx jy" of jitter_offset(k, P) as fp32 bit patterns in hex
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../basicrenderer_amd/csrc/brmi_temporal_math.h"

namespace tm = brmi::temporal;

template <typename T> static bool read_n(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "--jitter")) {
        const uint32_t n = (uint32_t)atoi(argv[2]), phases = (uint32_t)atoi(argv[3]);
        if (phases == 0u) return 2;
        for (uint32_t k = 0; k < n; k++) {
            float jx, jy;
            tm::jitter_offset(k, phases, jx, jy);
            printf("%08x %08x\n", brmi::display::bits_of(jx), brmi::display::bits_of(jy));
        }
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: temporal_main IN OUT | --jitter N PHASES\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[3]; float blend;
    if (fread(head, 4, 3, f) != 3 || fread(&blend, 4, 1, f) != 1 || head[0] == 0u || head[1] == 0u) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t W = head[0], H = head[1]; const bool haveHistory = head[2] != 0u;
    const size_t n = (size_t)W * H;
    std::vector<uint64_t> hdr, history, out(n); std::vector<float> depth; std::vector<uint32_t> motion;
    if (!read_n(f, hdr, n) || !read_n(f, depth, n) || !read_n(f, motion, n) || (haveHistory && !read_n(f, history, n))) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);
    auto words = [W](const std::vector<uint64_t>& img) { return [&img, W](uint32_t x, uint32_t y, uint32_t& lo, uint32_t& hi) { const uint64_t v = img[(size_t)y * W + x]; lo = (uint32_t)v; hi = (uint32_t)(v >> 32); }; };
    for (uint32_t y = 0; y < H; y++) for (uint32_t x = 0; x < W; x++) {
        uint32_t lo, hi;
        tm::resolve_pixel(x, y, W, H, blend, haveHistory, words(hdr), [&](uint32_t sx, uint32_t sy) { return depth[(size_t)sy * W + sx]; },
                          [&](uint32_t sx, uint32_t sy) { return motion[(size_t)sy * W + sx]; }, words(history), lo, hi);
        out[(size_t)y * W + x] = (uint64_t)lo | ((uint64_t)hi << 32);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(out.data(), 8, n, o) != n) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(o);
    return 0;
}
