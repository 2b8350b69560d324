// texture.h -- bitmap textures on a BSDF's reflectance, host + device, one
// source: the hit's texture coordinates (its.uv: rectangle.cpp:163 for a quad,
// skdtree.h:399-405 for a triangle) and Texture2D::eval(its, false)
// (mitsuba/src/librender/texture.cpp:112-121: uv * uvScale + uvOffset) over
// BitmapTexture::eval(uv) (textures/bitmap.cpp:431-454): MIPMap::evalBilinear
// or, with the nearest filter, evalBox, both on level 0, with evalTexel's five
// boundary rules on each axis separately (include/mitsuba/render/mipmap.h:
// 503-596), restated.  The camera and shade kernels of render.hip call it for
// the hit they traced, scene_texture_kernel and the host ABI
// sdmm_scene_texture_host run the same code (tests/test_texture_cases.py,
// tests/cpp/texture_check.cpp).  Float arithmetic without contraction, so that
// host and device agree bitwise.  No HIP include; under hipcc the functions
// are __host__ __device__.
//
// Departures:
//  - Mitsuba's camera rays carry differentials and default to the EWA lookup
//    (bitmap.cpp:486); this library has no ray differentials, every hit takes
//    eval(uv), as the reference's bounce rays do (the same departure as
//    envmap.h).
//  - A non-finite uv gives 0: evalBilinear's guard (mipmap.h:576-579), applied
//    in nearest mode too (evalBox has none).
//  - A texel coordinate whose floor does not fit int32 gives 0: the
//    reference's floorToInt is undefined there.
//  - The pixels are linear RGB as given: no flip, no gamma, no fromLinearRGB;
//    the caller decodes.  A negative or non-finite texel is rejected at scene
//    creation (the reference reads any bitmap).
// Not done: textured specular reflectance, exponent, alpha or radiance; EWA /
// trilinear filtering; computeShadingFrame's UV tangents; procedural textures;
// image-file reading.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mesh_intersect.h"

#if defined(__HIPCC__)
#define SDMM_TEX_HD __host__ __device__ __forceinline__
#else
#define SDMM_TEX_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sdmm {

constexpr int kTexBilinear = 0;
constexpr int kTexNearest = 1;
// ReconstructionFilter::EBoundaryCondition, in sdmm_texture's numbering
constexpr int kWrapRepeat = 0;
constexpr int kWrapClamp = 1;
constexpr int kWrapMirror = 2;
constexpr int kWrapZero = 3;
constexpr int kWrapOne = 4;
// all of a scene's textures together (so 2 * w, an index and x + 1 fit int32)
constexpr int64_t kTexMaxTexels = (int64_t)1 << 26;

// The device copy of a bitmap: one 16-byte RGBA texel (a unused), row major,
// row 0 is v = 0 -- a texel is one dwordx4 load, a bilinear lookup four.  The
// host entry reads the caller's [h][w][3] array in place (RGBA = false).
struct alignas(16) TexTexel {
    float r, g, b, a;
};
static_assert(sizeof(TexTexel) == 16, "TexTexel layout");

struct TextureDev {
    const float* texels;   // TexTexel[h * w] (device) or float[h * w * 3] (host)
    int w, h;
    int filter;            // kTexBilinear / kTexNearest
    int wrap_u, wrap_v;    // kWrap*
    float scale[2], offset[2];   // m_uvScale, m_uvOffset
};

// What a hit on a mesh reads for its uv (68 B), indexed by the caller's
// triangle index: the triangle as the test takes it (tri.id: that index), and
// its three vertices' texture coordinates (has_uv 0: the mesh has none, the
// hit's uv is the test's own (u, v), skdtree.h:403-405)
struct MeshUV {
    MeshTri tri;
    float t0[2], t1[2], t2[2];
    int32_t has_uv;
};
static_assert(sizeof(MeshUV) == 68, "MeshUV layout");

// its.uv of a triangle hit with the test's barycentrics u, v:
// t0 b.x + t1 b.y + t2 b.z, b = (1 - u - v, u, v) (skdtree.h:399-402)
SDMM_TEX_HD void tri_uv(const MeshUV& V, float u, float v, float uv[2]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!V.has_uv) {
        uv[0] = u;
        uv[1] = v;
        return;
    }
    const float b0 = 1.0f - u - v;
    for (int a = 0; a < 2; ++a) uv[a] = V.t0[a] * b0 + V.t1[a] * u + V.t2[a] * v;
}

// its.uv of the hit of the ray (o, d) on a quad (corner p0, unit normal n,
// duals g1, g2): the two parametric coordinates the closest-hit search forms
// (quads_closest, render_device.h: the same expressions on the same operands,
// so the same a, b it accepted) -- rectangle.cpp:163 with p0 as the local
// (-1, -1) corner.  A ray parallel to the quad: 0 (the search never reports it).
SDMM_TEX_HD void quad_uv(const float p0[3], const float n[3], const float g1[3], const float g2[3],
                         const float o[3], const float d[3], float uv[2]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    uv[0] = uv[1] = 0.0f;
    const float denom = d[0] * n[0] + d[1] * n[1] + d[2] * n[2];
    if (denom == 0.0f) return;
    const float r0[3] = {p0[0] - o[0], p0[1] - o[1], p0[2] - o[2]};
    const float t = (r0[0] * n[0] + r0[1] * n[1] + r0[2] * n[2]) / denom;
    const float r[3] = {o[0] + t * d[0] - p0[0], o[1] + t * d[1] - p0[1], o[2] + t * d[2] - p0[2]};
    uv[0] = r[0] * g1[0] + r[1] * g1[1] + r[2] * g1[2];
    uv[1] = r[0] * g2[0] + r[1] * g2[1] + r[2] * g2[2];
}

// its.uv of the hit of the ray (o, d) on primitive q (a quad, or n_quads +
// triangle): the search keeps only (primitive, t), so the primitive's test
// runs once more on the winner -- the same source on the same operands, as
// shading_normal.h does.  Quad: any record with p0, n, g1, g2 (QuadDev).  A ray
// the triangle test rejects: 0.
template <class Quad>
SDMM_TEX_HD void hit_uv(const Quad* quads, int n_quads, const MeshUV* mesh_uv, int q, const float o[3],
                        const float d[3], float uv[2]) {
    if (q >= n_quads) {
        const MeshUV& V = mesh_uv[q - n_quads];
        float t, u, v;
        uv[0] = uv[1] = 0.0f;
        if (tri_intersect_uv(V.tri, o, d, &t, &u, &v)) tri_uv(V, u, v, uv);
        return;
    }
    const Quad& Q = quads[q];
    quad_uv(Q.p0, Q.n, Q.g1, Q.g2, o, d, uv);
}

// evalTexel's boundary rule on one axis (mipmap.h:506-532): the texel index
// for coordinate x on an axis of n texels, or -1: the texel is `fill` (0 or 1)
SDMM_TEX_HD int tex_wrap(int x, int n, int wrap, float* fill) {
    if (x >= 0 && x < n) return x;
    switch (wrap) {
        case kWrapRepeat: {
            const int r = x % n;           // math::modulo
            return r < 0 ? r + n : r;
        }
        case kWrapClamp: return x < 0 ? 0 : n - 1;
        case kWrapMirror: {
            int r = x % (2 * n);
            if (r < 0) r += 2 * n;
            return r >= n ? 2 * n - r - 1 : r;
        }
        case kWrapZero: *fill = 0.0f; return -1;
        default: *fill = 1.0f; return -1;  // kWrapOne
    }
}

// evalTexel(0, x, y) (mipmap.h:503-563): the u axis decides first
template <bool RGBA>
SDMM_TEX_HD void tex_texel(const TextureDev& T, int x, int y, float c[3]) {
    float fill = 0.0f;
    const int xi = tex_wrap(x, T.w, T.wrap_u, &fill);
    if (xi < 0) {
        c[0] = c[1] = c[2] = fill;
        return;
    }
    const int yi = tex_wrap(y, T.h, T.wrap_v, &fill);
    if (yi < 0) {
        c[0] = c[1] = c[2] = fill;
        return;
    }
    const int64_t at = (int64_t)yi * T.w + xi;
    if constexpr (RGBA) {
        const TexTexel t = reinterpret_cast<const TexTexel*>(T.texels)[at];
        c[0] = t.r; c[1] = t.g; c[2] = t.b;
    } else {
        c[0] = T.texels[3 * at]; c[1] = T.texels[3 * at + 1]; c[2] = T.texels[3 * at + 2];
    }
}

// floor(x) as an int (math::floorToInt); false: it does not fit int32
SDMM_TEX_HD bool tex_floor(float x, int* i, float* f) {
    *f = floorf(x);
    if (!(*f >= -2147483648.0f && *f < 2147483648.0f)) return false;
    *i = (int)*f;
    return true;
}

// Texture2D::eval(its, false) for its.uv = uv_hit -> rgb
template <bool RGBA>
SDMM_TEX_HD void tex_eval(const TextureDev& T, const float uv_hit[2], float rgb[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    rgb[0] = rgb[1] = rgb[2] = 0.0f;
    const float uvx = uv_hit[0] * T.scale[0] + T.offset[0];
    const float uvy = uv_hit[1] * T.scale[1] + T.offset[1];
    if (!(fabsf(uvx) <= 3.402823466e38f) || !(fabsf(uvy) <= 3.402823466e38f)) return;   // evalBilinear's NaN guard
    int x, y;
    float fx, fy;
    if (T.filter == kTexNearest) {
        // evalBox (mipmap.h:566-569)
        if (!tex_floor(uvx * (float)T.w, &x, &fx) || !tex_floor(uvy * (float)T.h, &y, &fy)) return;
        tex_texel<RGBA>(T, x, y, rgb);
        return;
    }
    // evalBilinear (mipmap.h:585-595)
    const float u = uvx * (float)T.w - 0.5f, v = uvy * (float)T.h - 0.5f;
    if (!tex_floor(u, &x, &fx) || !tex_floor(v, &y, &fy)) return;
    const float dx1 = u - fx, dx2 = 1.0f - dx1, dy1 = v - fy, dy2 = 1.0f - dy1;
    float t00[3], t01[3], t10[3], t11[3];
    tex_texel<RGBA>(T, x, y, t00);
    tex_texel<RGBA>(T, x, y + 1, t01);
    tex_texel<RGBA>(T, x + 1, y, t10);
    tex_texel<RGBA>(T, x + 1, y + 1, t11);
    for (int ch = 0; ch < 3; ++ch)
        rgb[ch] = t00[ch] * dx2 * dy2 + t01[ch] * dx2 * dy1 + t10[ch] * dx1 * dy2 + t11[ch] * dx1 * dy1;
}

}  // namespace sdmm
