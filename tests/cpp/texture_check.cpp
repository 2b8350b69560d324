// texture_check.cpp -- the bitmap lookup (csrc/texture.h) as a stand-alone
// program for a sanitizer build (tests/test_texture_cases.py): the textures
// and texture coordinates of the Python tests from a fixture file, every
// texture against every uv through tex_eval -- reading the [h][w][3] array in
// place and, as the device does, a copy of RGBA texels; the two must agree.
// Then the uv helpers on a few hand-made hits.  Writes the colours to
// <fixture>.out ([n_textures][nq][3] float32), which the test compares with
// its numpy restatement bitwise.
//
// Fixture: int32 n_textures, nq; float uv[nq][2]; per texture: int32 w, h,
// filter, wrap_u, wrap_v; float scale[2], offset[2]; float pixels[h][w][3].
#include <xmmintrin.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "texture.h"

using namespace sdmm;

namespace {
struct Quad {
    float p0[3], n[3], g1[3], g2[3];
};
int fail(const char* what) {
    std::printf("texture_check: %s\n", what);
    return 1;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: texture_check <fixture file>\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[2];
    if (std::fread(hdr, sizeof(int32_t), 2, f) != 2 || hdr[0] < 1 || hdr[1] < 1) return 2;
    const int n_tex = hdr[0];
    const size_t nq = (size_t)hdr[1];
    std::vector<float> uv(nq * 2);
    if (std::fread(uv.data(), sizeof(float), uv.size(), f) != uv.size()) return 2;
    // the library's float environment: denormals flushed, as on the device
    _mm_setcsr(_mm_getcsr() | 0x8040u);
    std::vector<float> out;
    out.reserve((size_t)n_tex * nq * 3);
    for (int k = 0; k < n_tex; ++k) {
        int32_t ih[5];
        float fh[4];
        if (std::fread(ih, sizeof(int32_t), 5, f) != 5 || std::fread(fh, sizeof(float), 4, f) != 4) return 2;
        TextureDev T{};
        T.w = ih[0];
        T.h = ih[1];
        T.filter = ih[2];
        T.wrap_u = ih[3];
        T.wrap_v = ih[4];
        for (int a = 0; a < 2; ++a) {
            T.scale[a] = fh[a];
            T.offset[a] = fh[2 + a];
        }
        if (T.w < 1 || T.h < 1) return 2;
        // exactly the bitmap's size: a texel index out of range is a heap overflow the sanitizer reports
        std::vector<float> px((size_t)T.w * (size_t)T.h * 3);
        if (std::fread(px.data(), sizeof(float), px.size(), f) != px.size()) return 2;
        std::vector<TexTexel> rgba((size_t)T.w * (size_t)T.h);
        for (size_t i = 0; i < rgba.size(); ++i) rgba[i] = TexTexel{px[3 * i], px[3 * i + 1], px[3 * i + 2], 0.0f};
        TextureDev R = T;
        T.texels = px.data();
        R.texels = reinterpret_cast<const float*>(rgba.data());
        for (size_t i = 0; i < nq; ++i) {
            float a[3], b[3];
            tex_eval<false>(T, &uv[2 * i], a);
            tex_eval<true>(R, &uv[2 * i], b);
            if (std::memcmp(a, b, sizeof a) != 0) return fail("the in-place and the RGBA lookup differ");
            for (int c = 0; c < 3; ++c) {
                if (!(a[c] >= 0.0f)) return fail("a negative or NaN colour");
                out.push_back(a[c]);
            }
        }
    }
    std::fclose(f);
    // the uv helpers: a unit quad in y = 0 and the triangle (0,0,0) (1,0,0) (0,0,1), met from above
    const Quad Q{{0, 0, 0}, {0, -1, 0}, {1, 0, 0}, {0, 0, 1}};
    MeshUV V{};
    V.tri = MeshTri{{0, 0, 0}, {1, 0, 0}, {0, 0, 1}, 0};
    const float tcs[3][2] = {{-0.5f, 2.0f}, {1.5f, 2.0f}, {-0.5f, 4.0f}};
    for (int a = 0; a < 2; ++a) {
        V.t0[a] = tcs[0][a];
        V.t1[a] = tcs[1][a];
        V.t2[a] = tcs[2][a];
    }
    const float d[3] = {0.0f, -1.0f, 0.0f};
    for (int i = 0; i <= 4; ++i)
        for (int j = 0; i + j <= 4; ++j) {
            const float o[3] = {0.25f * i, 1.0f, 0.25f * j};
            float q[2], b[2], t[2];
            hit_uv(&Q, 1, &V, 0, o, d, q);
            if (q[0] != o[0] || q[1] != o[2]) return fail("a quad's uv is not (a, b)");
            V.has_uv = 0;
            hit_uv(&Q, 1, &V, 1, o, d, b);
            if (b[0] != o[0] || b[1] != o[2]) return fail("a bare triangle's uv is not (u, v)");
            V.has_uv = 1;
            hit_uv(&Q, 1, &V, 1, o, d, t);
            if (t[0] != -0.5f + 2.0f * o[0] || t[1] != 2.0f + 2.0f * o[2]) return fail("a triangle's interpolated uv");
        }
    {
        // rays the primitive's test rejects: 0
        const float o[3] = {0.25f, 1.0f, 0.25f}, along[3] = {1.0f, 0.0f, 0.0f};
        float q[2] = {7, 7}, t[2] = {7, 7};
        hit_uv(&Q, 1, &V, 0, o, along, q);
        hit_uv(&Q, 1, &V, 1, o, along, t);
        if (q[0] != 0 || q[1] != 0 || t[0] != 0 || t[1] != 0) return fail("a rejected ray's uv is not 0");
    }
    std::FILE* g = std::fopen((std::string(argv[1]) + ".out").c_str(), "wb");
    if (!g) return 2;
    std::fwrite(out.data(), sizeof(float), out.size(), g);
    std::fclose(g);
    std::printf("texture_check ok: %d textures, %zu uvs\n", n_tex, nq);
    return 0;
}
