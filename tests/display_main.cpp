// display_main.cpp -- brmi_display_math.h on the host, for tests/test_display_cpu.py: reads fixed inputs, prints what the header computes as JSON.
//   display_main <inputs.bin>
//   display_main --properties <props.bin>
// inputs.bin: u32 n, then n x 3 floats (colours); u32 m, then m floats (adapted luminances); 256 u32 (a histogram), float numPixels; u32 t, then t x 13 and
// t x 9 floats (tap values of one channel).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../basicrenderer_amd/csrc/brmi_display_math.h"

namespace dm = brmi::display;

static void put(const char* name, const std::vector<double>& v, bool last = false) {
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) std::printf("%s%.9g", i ? ", " : "", v[i]);
    std::printf("]%s\n", last ? "" : ",");
}
static void put_u(const char* name, const std::vector<uint32_t>& v) {
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) std::printf("%s%u", i ? ", " : "", v[i]);
    std::printf("],\n");
}
template <typename T> static std::vector<T> read_n(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return v;
}

// display_main --properties <props.bin>: the inputs of the property tests through the header.  props.bin: u32 a, a floats (adapted luminances); u32 g, g floats
// (greys); u32 w, w x 3 floats (colours); u32 c, c floats (constants); u32 h, h x (256 u32, float numPixels) (histograms); u32 f, f floats (for half_bits).
static int properties(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    const std::vector<float> adapted = read_n<float>(f, read_n<uint32_t>(f, 1)[0]);
    const std::vector<float> greys = read_n<float>(f, read_n<uint32_t>(f, 1)[0]);
    const std::vector<float> wide = read_n<float>(f, 3u * read_n<uint32_t>(f, 1)[0]);
    const std::vector<float> consts = read_n<float>(f, read_n<uint32_t>(f, 1)[0]);
    const uint32_t nh = read_n<uint32_t>(f, 1)[0];
    std::vector<uint32_t> sums;
    std::vector<double> averages;
    const float minLog = dm::kMinLogLuminance, range = dm::default_log_luminance_range();
    for (uint32_t i = 0; i < nh; i++) {
        const std::vector<uint32_t> hist = read_n<uint32_t>(f, 256);
        const float numPixels = read_n<float>(f, 1)[0];
        sums.push_back(dm::weighted_sum(hist.data()));
        averages.push_back(dm::average_luminance(sums.back(), hist[0], numPixels, minLog, range));
    }
    const std::vector<float> unrounded = read_n<float>(f, read_n<uint32_t>(f, 1)[0]);
    std::fclose(f);
    std::printf("{\n");
    std::vector<double> midIn, lpmMid, lpmMax;
    for (float a : adapted) {
        const dm::LpmParams p = dm::lpm_params(a);
        const float mid = (dm::kHdrMax * 0.18f) * exp2f(-dm::exposure_of(a));
        midIn.push_back(mid);
        const dm::rgb lo = dm::lpm_map(dm::rgb{mid, mid, mid}, p), hi = dm::lpm_map(dm::rgb{dm::kHdrMax, dm::kHdrMax, dm::kHdrMax}, p);
        lpmMid.push_back(lo.r); lpmMid.push_back(lo.g); lpmMid.push_back(lo.b);
        lpmMax.push_back(hi.r); lpmMax.push_back(hi.g); lpmMax.push_back(hi.b);
    }
    put("midIn", midIn); put("lpmMid", lpmMid); put("lpmMax", lpmMax);
    const dm::LpmParams lpm = dm::lpm_params(0.5f);
    const char* names[5] = {"rampReinhard", "rampNeutral", "rampAces", "rampLpm", "rampNone"};
    for (uint32_t curve = 0; curve < 5u; curve++) {
        std::vector<double> ramp;
        for (float g : greys) ramp.push_back(dm::tone_map_of(curve, dm::rgb{g, g, g}, lpm).g);
        put(names[curve], ramp);
    }
    std::vector<double> aces, none;
    std::vector<uint32_t> noneCodes, halves;
    for (size_t i = 0; i + 2 < wide.size(); i += 3) {
        const dm::rgb c{wide[i], wide[i + 1], wide[i + 2]};
        const dm::rgb a = dm::tone_map_of(2u, c, lpm), n = dm::tone_map_of(4u, c, lpm);
        aces.push_back(a.r); aces.push_back(a.g); aces.push_back(a.b);
        none.push_back(n.r); none.push_back(n.g); none.push_back(n.b);
        const uint32_t px = dm::ldr_pixel(n);
        noneCodes.push_back(px & 255u); noneCodes.push_back((px >> 8) & 255u); noneCodes.push_back((px >> 16) & 255u); noneCodes.push_back(px >> 24);
    }
    put("aces", aces); put("none", none); put_u("noneCodes", noneCodes);
    std::vector<double> constDown, constTent;
    for (float c : consts) {
        float t13[13], t9[9];
        for (float& x : t13) x = c;
        for (float& x : t9) x = c;
        const float v = dm::bloom_down_combine(t13);
        dm::rgb out{v, v, v};
        const bool kept = dm::bloom_down_tail(out);
        constDown.push_back(kept ? 1.0 : 0.0); constDown.push_back(out.r); constDown.push_back(out.g); constDown.push_back(out.b);
        constTent.push_back(dm::bloom_tent_combine(t9));
    }
    put("constDown", constDown); put("constTent", constTent);
    put_u("histSums", sums); put("histAverages", averages);
    for (float x : unrounded) halves.push_back(dm::half_bits(x));
    put_u("halfBits", halves);
    std::printf("\"done\": [1]\n}\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (argc >= 3 && std::string(argv[1]) == "--properties") return properties(argv[2]);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const uint32_t n = read_n<uint32_t>(f, 1)[0];
    const std::vector<float> colours = read_n<float>(f, 3u * n);
    const uint32_t m = read_n<uint32_t>(f, 1)[0];
    const std::vector<float> adapted = read_n<float>(f, m);
    const std::vector<uint32_t> hist = read_n<uint32_t>(f, 256);
    const float numPixels = read_n<float>(f, 1)[0];
    const uint32_t t = read_n<uint32_t>(f, 1)[0];
    const std::vector<float> down = read_n<float>(f, 13u * t), tent = read_n<float>(f, 9u * t);
    std::fclose(f);
    const float minLog = dm::kMinLogLuminance, range = dm::default_log_luminance_range(), invRange = 1.0f / range;

    std::printf("{\n");
    std::vector<uint32_t> bins, codes, halves;
    for (uint32_t i = 0; i < n; i++) bins.push_back(dm::luminance_bin(colours[3 * i], colours[3 * i + 1], colours[3 * i + 2], minLog, invRange));
    put_u("bins", bins);
    put_u("weightedSum", {dm::weighted_sum(hist.data())});
    const float average = dm::average_luminance(dm::weighted_sum(hist.data()), hist[0], numPixels, minLog, range);
    put("average", {average, dm::adapt_luminance(0.5f, average, 0.25f)});
    std::vector<double> control, mapped[5];
    for (uint32_t k = 0; k < m; k++) {
        uint32_t ctl[96];
        dm::lpm_setup(adapted[k], ctl);
        for (int w = 0; w < 96; w++) control.push_back(dm::float_of(ctl[w]));
    }
    put("control", control);
    const dm::LpmParams lpm = dm::lpm_params(adapted.empty() ? 0.18f : adapted[0]);
    for (uint32_t curve = 0; curve < 5u; curve++)
        for (uint32_t i = 0; i < n; i++) {
            const dm::rgb o = dm::tone_map_of(curve, dm::rgb{colours[3 * i], colours[3 * i + 1], colours[3 * i + 2]}, lpm);
            mapped[curve].push_back(o.r); mapped[curve].push_back(o.g); mapped[curve].push_back(o.b);
            if (curve == 4u) { const uint32_t px = dm::ldr_pixel(o); codes.push_back(px & 255u); codes.push_back((px >> 8) & 255u); codes.push_back((px >> 16) & 255u); codes.push_back(px >> 24); }
        }
    put("reinhard", mapped[0]); put("neutral", mapped[1]); put("aces", mapped[2]); put("lpm", mapped[3]); put("none", mapped[4]);
    put_u("codes", codes);
    for (uint32_t i = 0; i < 3u * n; i++) halves.push_back(dm::half_bits(colours[i]));
    put_u("halves", halves);
    std::vector<double> downs, tents, tails;
    for (uint32_t i = 0; i < t; i++) { downs.push_back(dm::bloom_down_combine(&down[13 * i])); tents.push_back(dm::bloom_tent_combine(&tent[9 * i])); }
    for (uint32_t i = 0; i + 2 < t; i += 3) {
        dm::rgb v{(float)downs[i], (float)downs[i + 1], (float)downs[i + 2]};
        const bool kept = dm::bloom_down_tail(v);
        tails.push_back(kept ? 1.0 : 0.0); tails.push_back(v.r); tails.push_back(v.g); tails.push_back(v.b);
    }
    put("down", downs); put("tent", tents); put("tail", tails);
    std::vector<uint32_t> levels;
    const uint32_t sizes[3][2] = {{64, 40}, {101, 53}, {40, 24}};
    for (auto& s : sizes) {
        levels.push_back(dm::bloom_level_count(s[0], s[1])); levels.push_back(dm::bloom_possible(s[0], s[1]) ? 1u : 0u);
        for (uint32_t l = 1; l <= 5u; l++) { levels.push_back(dm::bloom_level_size(s[0], l)); levels.push_back(dm::bloom_level_size(s[1], l)); }
    }
    put_u("levels", levels);
    put("blend", {dm::bloom_blend(1.5f, 3.25f), dm::bloom_add(0.333251953125f, 1.0009765625f)}, true);
    std::printf("}\n");
    return 0;
}
