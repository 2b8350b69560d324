// bsdf_phong.h -- the modified Phong BSDF (mitsuba/src/bsdfs/phong.cpp:
// 171-289) in the local shading frame, host + device: the device Li's loop
// head samples it, its shade kernel evaluates it, and the host ABI
// sdmm_bsdf_phong_host runs the same code (tests/test_learned_nd.py checks it
// against the formulas in float64).  bp: the BSDF's 8 bsdf_params floats --
// [1..3] specularReflectance, [4] exponent, [5] the specular sampling weight;
// rho: its diffuseReflectance.  Float arithmetic without contraction; pow /
// sin / cos as (float)f((double)x), like the library's other BSDF code.
// Frame(n) and the cosine-hemisphere warp, which Phong's sampling shares with
// render.hip's other BSDFs, live here too (host + device for that reason).
#pragma once
#include <hip/hip_runtime.h>

namespace sdmm {

// Frame(n): Mitsuba coordinateSystem (s, t, n)
__host__ __device__ __forceinline__ void frame_of(const float n[3], float s[3], float t[3]) {
#pragma clang fp contract(off)
    if (fabsf(n[0]) > fabsf(n[1])) {
        const float inv = 1.0f / sqrtf(n[0] * n[0] + n[2] * n[2]);
        t[0] = n[2] * inv; t[1] = 0.0f; t[2] = -n[0] * inv;
    } else {
        const float inv = 1.0f / sqrtf(n[1] * n[1] + n[2] * n[2]);
        t[0] = 0.0f; t[1] = n[2] * inv; t[2] = -n[1] * inv;
    }
    s[0] = t[1] * n[2] - t[2] * n[1];
    s[1] = t[2] * n[0] - t[0] * n[2];
    s[2] = t[0] * n[1] - t[1] * n[0];
}

// warp::squareToCosineHemisphere (concentric disk, z guarded to 1e-10)
__host__ __device__ __forceinline__ void cosine_hemisphere(float u0, float u1, float w[3]) {
#pragma clang fp contract(off)
    constexpr double kPiD = 3.14159265358979323846;
    const float r1 = 2.0f * u0 - 1.0f, r2 = 2.0f * u1 - 1.0f;
    float r, phi;
    if (r1 == 0.0f && r2 == 0.0f) {
        r = 0.0f; phi = 0.0f;
    } else if (r1 * r1 > r2 * r2) {
        r = r1; phi = (float)(kPiD / 4.0) * (r2 / r1);
    } else {
        r = r2; phi = (float)(kPiD / 2.0) - (r1 / r2) * (float)(kPiD / 4.0);
    }
    // sin / cos in double, rounded: the float values the CPU restatement
    // (oracle/sdmm_oracle_li.inc) forms with the C library
    double sd, cd;
    sincos((double)phi, &sd, &cd);
    const float sp = (float)sd, cp = (float)cd;
    w[0] = r * cp;
    w[1] = r * sp;
    float z = sqrtf(fmaxf(0.0f, 1.0f - w[0] * w[0] - w[1] * w[1]));
    if (z == 0.0f) z = 1e-10f;
    w[2] = z;
}

// Phong::eval (ESolidAngle, :171-196) into f and Phong::pdf (:198-230), both
// lobes enabled
__host__ __device__ __forceinline__ float phong_eval_pdf(const float wi[3], const float wo[3], const float* bp,
                                                         const float rho[3], float f[3]) {
#pragma clang fp contract(off)
    constexpr float kInvPiF = 0.31830988618379067154f, kInvTwoPiF = 0.15915494309189533577f;
    constexpr float kTwoPiF = 6.28318530717958647692f;
    f[0] = f[1] = f[2] = 0.0f;
    if (wi[2] <= 0.0f || wo[2] <= 0.0f) return 0.0f;
    const float exponent = bp[4], ssw = bp[5];
    // dot(wo, reflect(wi)), reflect(wi) = (-wi.x, -wi.y, wi.z)
    const float alpha = wo[0] * -wi[0] + wo[1] * -wi[1] + wo[2] * wi[2];
    float spec = 0.0f, spec_prob = 0.0f;
    if (alpha > 0.0f) {
        const float pa = (float)pow((double)alpha, (double)exponent);
        spec = (exponent + 2.0f) * kInvTwoPiF * pa;
        spec_prob = pa * (exponent + 1.0f) / kTwoPiF;
    }
    for (int ch = 0; ch < 3; ++ch) f[ch] = (bp[1 + ch] * spec + rho[ch] * kInvPiF) * wo[2];
    return ssw * spec_prob + (1.0f - ssw) * (kInvPiF * wo[2]);
}

// Phong::sample(bRec, pdf, sample) (:232-289), wi.z > 0: wo, the weight eval /
// pdf and the solid-angle pdf; false: the sample is void (weight 0, pdf 0).
// u0 <= weight picks the specular lobe -- not with weight 0, where the
// reference divides 0 by 0 at u0 = 0 (a NaN direction for a lobe of no energy).
__host__ __device__ __forceinline__ bool phong_sample(const float wi[3], const float* bp, const float rho[3],
                                                      float u0, float u1, float wo[3], float bw[3], float* pdf) {
#pragma clang fp contract(off)
    constexpr float kTwoPiF = 6.28318530717958647692f;
    const float exponent = bp[4], ssw = bp[5];
    *pdf = 0.0f;
    bw[0] = bw[1] = bw[2] = 0.0f;
    if (u0 <= ssw && ssw > 0.0f) {
        u0 = u0 / ssw;
        const float R[3] = {-wi[0], -wi[1], wi[2]};
        // a Phong lobe about (0, 0, 1), rotated into Frame(R)
        const float sin_a = sqrtf(1.0f - (float)pow((double)u1, (double)(2.0f / (exponent + 1.0f))));
        const float cos_a = (float)pow((double)u1, (double)(1.0f / (exponent + 1.0f)));
        const float phi = kTwoPiF * u0;
        double sd, cd;
        sincos((double)phi, &sd, &cd);
        const float l[3] = {sin_a * (float)cd, sin_a * (float)sd, cos_a};
        float s[3], t[3];
        frame_of(R, s, t);
        for (int a = 0; a < 3; ++a) wo[a] = s[a] * l[0] + t[a] * l[1] + R[a] * l[2];
        if (wo[2] <= 0.0f) return false;
    } else {
        cosine_hemisphere((u0 - ssw) / (1.0f - ssw), u1, wo);
    }
    float f[3];
    const float p = phong_eval_pdf(wi, wo, bp, rho, f);
    if (p == 0.0f) return false;
    // Spectrum / pdf (TSpectrum::operator/: times the reciprocal)
    const float rp = 1.0f / p;
    for (int ch = 0; ch < 3; ++ch) bw[ch] = f[ch] * rp;
    *pdf = p;
    return true;
}

}  // namespace sdmm
