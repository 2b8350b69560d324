// exr_check.cpp -- sdmm_read_exr as a stand-alone program over the library
// (tests/test_film.py), also the form a sanitizer build of the reader takes:
// the first file must read back (size query, then the planes into a buffer of
// exactly that size), every further file is one of the malformed family and
// must be refused with SDMM_E_INVALID and a message, at the size query or,
// where its header is whole, at the read.
#include <cstdio>
#include <cstring>
#include <vector>

#include "sdmm_gpu.h"

static int read_file(const char* path, std::vector<float>& rgb, int* w, int* h) {
    int spp = -1, iteration = -1;
    float time = -1.0f;
    int rc = sdmm_read_exr(path, w, h, nullptr, &spp, &iteration, &time);
    if (rc != SDMM_OK) return rc;
    if (*w < 1 || *h < 1 || (long long)*w * *h > (1ll << 26)) return 100;
    rgb.assign((size_t)3 * (size_t)*w * (size_t)*h, 0.0f);
    return sdmm_read_exr(path, w, h, rgb.data(), &spp, &iteration, &time);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: exr_check <good file> [malformed files...]\n");
        return 2;
    }
    std::vector<float> rgb;
    int w = 0, h = 0;
    int rc = read_file(argv[1], rgb, &w, &h);
    if (rc != SDMM_OK) {
        std::printf("%s: not read: %d %s\n", argv[1], rc, sdmm_last_error());
        return 1;
    }
    int refused = 0;
    for (int i = 2; i < argc; ++i) {
        rc = read_file(argv[i], rgb, &w, &h);
        const char* msg = sdmm_last_error();
        if (rc != SDMM_E_INVALID || !msg || !std::strlen(msg)) {
            std::printf("%s: expected SDMM_E_INVALID with a message, got %d\n", argv[i], rc);
            return 1;
        }
        ++refused;
    }
    std::printf("exr_check ok: 1 read, %d refused\n", refused);
    return 0;
}
