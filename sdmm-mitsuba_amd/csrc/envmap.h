// envmap.h -- the environment emitter of the device Li, host + device, one
// source: Emitter::evalEnvironment of a `constant` emitter (mitsuba/src/
// emitters/constant.cpp: the radiance, whatever the direction) and of a
// lat-long `envmap` (emitters/envmap.cpp:380-393, :409 over MIPMap::
// evalBilinear, include/mitsuba/render/mipmap.h:575-596, ERepeat horizontally
// and EClamp vertically).  The camera and shade kernels of render.hip call it
// where a ray leaves the scene, env_eval_kernel and the host ABI
// sdmm_env_eval_host run the same code (tests/test_env.py, tests/cpp/
// env_check.cpp).  Float arithmetic without contraction; atan2 / acos as
// (float)f((double)x), like the library's BSDF code, so that host and device
// agree bitwise.  No HIP include; under hipcc the functions are __host__
// __device__.
//
// Departure: Mitsuba's camera rays carry differentials and take the
// EWA-filtered lookup (envmap.cpp:394-407); this library has no ray
// differentials, every ray takes the bilinear lookup (as the reference's
// bounce rays do).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SDMM_ENV_HD __host__ __device__ __forceinline__
#else
#define SDMM_ENV_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sdmm {

constexpr int kEnvNone = 0;
constexpr int kEnvConstant = 1;
constexpr int kEnvLatLong = 2;
constexpr int64_t kEnvMaxTexels = (int64_t)1 << 26;

// The device copy of a map: one 16-byte RGBA texel (a unused), row major, row
// 0 the +y pole -- a texel is one dwordx4 load, a lookup four.  The host
// entry reads the caller's [h][w][3] array in place (RGBA = false below).
struct alignas(16) EnvTexel {
    float r, g, b, a;
};
static_assert(sizeof(EnvTexel) == 16, "EnvTexel layout");

struct EnvDev {
    const float* texels;   // kind 2: EnvTexel[h * w] (device) or float[h * w * 3] (host)
    int kind;              // kEnvNone / kEnvConstant / kEnvLatLong
    int w, h;
    float scale;           // kind 2: m_scale
    float rad[3];          // kind 1: the radiance
    float m[9];            // kind 2: the linear part of toWorld.inverse(), row major
};

template <bool RGBA>
SDMM_ENV_HD void env_texel(const float* texels, int w, int x, int y, float c[3]) {
    const int64_t at = (int64_t)y * w + x;
    if constexpr (RGBA) {
        const EnvTexel t = reinterpret_cast<const EnvTexel*>(texels)[at];
        c[0] = t.r; c[1] = t.g; c[2] = t.b;
    } else {
        c[0] = texels[3 * at]; c[1] = texels[3 * at + 1]; c[2] = texels[3 * at + 2];
    }
}

// evalEnvironment for the world direction d (taken as given: no
// renormalisation, envmap.cpp:382) -> rgb.  kEnvNone: 0.
template <bool RGBA>
SDMM_ENV_HD void env_eval(const EnvDev& E, const float d[3], float rgb[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    rgb[0] = rgb[1] = rgb[2] = 0.0f;
    if (E.kind == kEnvConstant) {
        rgb[0] = E.rad[0]; rgb[1] = E.rad[1]; rgb[2] = E.rad[2];
        return;
    }
    if (E.kind != kEnvLatLong) return;
    constexpr float kInvTwoPi = 0.15915494309189533577f, kInvPiF = 0.31830988618379067154f;
    const float vx = E.m[0] * d[0] + E.m[1] * d[1] + E.m[2] * d[2];
    const float vy = E.m[3] * d[0] + E.m[4] * d[1] + E.m[5] * d[2];
    const float vz = E.m[6] * d[0] + E.m[7] * d[1] + E.m[8] * d[2];
    // math::safe_acos: std::min(1.0f, std::max(-1.0f, v.y)) -- a NaN becomes -1
    float cy = (-1.0f < vy) ? vy : -1.0f;
    cy = (cy < 1.0f) ? cy : 1.0f;
    const float uvx = (float)atan2((double)vx, (double)-vz) * kInvTwoPi;
    const float uvy = (float)acos((double)cy) * kInvPiF;
    if (!(fabsf(uvx) <= 3.402823466e38f) || !(fabsf(uvy) <= 3.402823466e38f)) return;   // evalBilinear's NaN guard
    const float u = uvx * (float)E.w - 0.5f, t = uvy * (float)E.h - 0.5f;
    const float fx = floorf(u), fy = floorf(t);
    const int x = (int)fx, y = (int)fy;
    const float dx1 = u - fx, dx2 = 1.0f - dx1, dy1 = t - fy, dy2 = 1.0f - dy1;
    // ERepeat: a positive modulo; EClamp: to [0, h - 1]
    int x0 = x % E.w;
    if (x0 < 0) x0 += E.w;
    int x1 = (x0 + 1) % E.w;
    const int y0 = y < 0 ? 0 : (y > E.h - 1 ? E.h - 1 : y);
    const int yp = y + 1;
    const int y1 = yp < 0 ? 0 : (yp > E.h - 1 ? E.h - 1 : yp);
    float t00[3], t01[3], t10[3], t11[3];
    env_texel<RGBA>(E.texels, E.w, x0, y0, t00);
    env_texel<RGBA>(E.texels, E.w, x0, y1, t01);
    env_texel<RGBA>(E.texels, E.w, x1, y0, t10);
    env_texel<RGBA>(E.texels, E.w, x1, y1, t11);
    for (int ch = 0; ch < 3; ++ch) {
        const float v = t00[ch] * dx2 * dy2 + t01[ch] * dx2 * dy1 + t10[ch] * dx1 * dy2 + t11[ch] * dx1 * dy1;
        rgb[ch] = v * E.scale;
    }
}

}  // namespace sdmm
