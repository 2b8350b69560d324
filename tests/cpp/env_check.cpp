// env_check.cpp -- the environment lookup (csrc/envmap.h) as a stand-alone
// program for a sanitizer build (tests/test_env.py): the maps and directions
// of the Python tests from a fixture file, every map against every direction.
// Writes the radiances to <fixture>.out ([n_maps][nq][3] float32), which the
// test compares with the library's bitwise.
//
// Fixture: int32 n_maps, nq; float d[nq][3]; per map: int32 kind, w, h; float
// scale, rad[3], m[9]; float pixels[h][w][3] (kind 2 only).
#include <xmmintrin.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "envmap.h"

using namespace sdmm;

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: env_check <fixture file>\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[2];
    if (std::fread(hdr, sizeof(int32_t), 2, f) != 2 || hdr[0] < 1 || hdr[1] < 1) return 2;
    const int n_maps = hdr[0];
    const size_t nq = (size_t)hdr[1];
    std::vector<float> d(nq * 3);
    if (std::fread(d.data(), sizeof(float), d.size(), f) != d.size()) return 2;
    // the library's float environment: denormals flushed, as on the device
    _mm_setcsr(_mm_getcsr() | 0x8040u);
    std::vector<float> out;
    for (int k = 0; k < n_maps; ++k) {
        int32_t ih[3];
        float fh[13];
        if (std::fread(ih, sizeof(int32_t), 3, f) != 3 || std::fread(fh, sizeof(float), 13, f) != 13) return 2;
        EnvDev E{};
        E.kind = ih[0];
        E.w = ih[1];
        E.h = ih[2];
        E.scale = fh[0];
        for (int i = 0; i < 3; ++i) E.rad[i] = fh[1 + i];
        for (int i = 0; i < 9; ++i) E.m[i] = fh[4 + i];
        // exactly the map's size: a texel index out of range is a heap overflow the sanitizer reports
        std::vector<float> px;
        if (E.kind == kEnvLatLong) {
            if (E.w < 1 || E.h < 1) return 2;
            px.resize((size_t)E.w * (size_t)E.h * 3);
            if (std::fread(px.data(), sizeof(float), px.size(), f) != px.size()) return 2;
            E.texels = px.data();
        }
        int nonzero = 0;
        for (size_t i = 0; i < nq; ++i) {
            float rgb[3];
            env_eval<false>(E, &d[3 * i], rgb);
            for (int c = 0; c < 3; ++c) {
                if (!(rgb[c] >= 0.0f)) {
                    std::printf("map %d, direction %zu: radiance %g\n", k, i, rgb[c]);
                    return 1;
                }
                out.push_back(rgb[c]);
            }
            nonzero += rgb[0] != 0.0f || rgb[1] != 0.0f || rgb[2] != 0.0f;
        }
        std::printf("map %d: kind %d, %d x %d, %zu directions, %d non-zero\n", k, E.kind, E.w, E.h, nq, nonzero);
    }
    std::fclose(f);
    std::FILE* g = std::fopen((std::string(argv[1]) + ".out").c_str(), "wb");
    if (!g) return 2;
    std::fwrite(out.data(), sizeof(float), out.size(), g);
    std::fclose(g);
    std::printf("env_check ok\n");
    return 0;
}
