// bsdf_roughdielectric.h -- the rough dielectric BSDF (mitsuba/src/bsdfs/
// roughdielectric.cpp: eval :317-395, pdf :397-469, sample(bRec, pdf, sample)
// :560-662) in the local shading frame, host + device: the device Li's loop
// head samples it, its shade kernel evaluates it, and the host ABI
// sdmm_bsdf_roughdielectric_host and the batch kernel behind
// sdmm_bsdf_roughdielectric_device run the same code
// (tests/test_bsdf_roughdielectric.py checks it against the formulas in
// float64).  Isotropic Beckmann, sampleVisible = false (bsdf_beckmann.h), both
// components enabled, ERadiance transport.
//
// bp: the BSDF's 8 bsdf_params floats -- [1..3] specularReflectance, [4] eta =
// intIOR / extIOR, [5] 1 / eta, [6] alpha; st: its specularTransmittance (the
// BSDF's `reflectance` row).  wi.z < 0 is a hit from inside: the interface is
// two-sided, eta or 1 / eta by the side.  wi.z == 0 evaluates and samples to 0
// (eval :318; the reference's sample divides by cosTheta(wi) there).
//
// Inputs and outputs are floats; the arithmetic between them is double,
// without contraction.  In float the reference's formulas miss their own
// float64 values by 1e-4 .. 2e-3 where they cancel -- sin theta_m = sqrt(1 -
// cos^2 theta_m) against the Beckmann exponent at small alpha, cosThetaT near
// the critical angle, wo.z and wo.m at grazing directions (smithG1, the
// half-vector Jacobian) -- and a rough interface meets all three on ordinary
// paths; in double the results are the float64 values rounded once.
#pragma once
#include <hip/hip_runtime.h>

#include "bsdf_beckmann.h"

namespace sdmm {

// fresnelDielectricExt with the cosThetaT output (libcore/util.cpp:651-681):
// the unpolarised reflectance at cos(theta_i) for the relative index eta (!=
// 1); *cos_t the transmitted cosine, signed against cos_i, 0 at a total
// internal reflection
__host__ __device__ __forceinline__ double fresnel_dielectric_ext(double cos_i, double eta, double* cos_t) {
#pragma clang fp contract(off)
    const double scale = cos_i > 0.0 ? 1.0 / eta : eta;
    const double ct2 = 1.0 - (1.0 - cos_i * cos_i) * (scale * scale);
    if (ct2 <= 0.0) {
        *cos_t = 0.0;
        return 1.0;
    }
    const double ci = fabs(cos_i), ct = sqrt(ct2);
    const double rs = (ci - eta * ct) / (ci + eta * ct);
    const double rp = (eta * ci - ct) / (eta * ci + ct);
    *cos_t = cos_i > 0.0 ? -ct : ct;
    return 0.5 * (rs * rs + rp * rp);
}

// The Walter trick (:453-458, :492-498): the sampling distribution's alpha
__host__ __device__ __forceinline__ double roughdielectric_sample_alpha(double alpha, double cos_i) {
#pragma clang fp contract(off)
    return alpha * (1.2 - 0.2 * sqrt(fabs(cos_i)));
}

// The relative index a direction crosses (bRec.eta of sample, :615, :633): 1
// on reflection, eta entering (wi.z > 0), 1 / eta leaving
__host__ __device__ __forceinline__ float roughdielectric_crossed_eta(const float wi[3], const float wo[3],
                                                                      const float* bp) {
#pragma clang fp contract(off)
    if ((double)wi[2] * (double)wo[2] > 0.0) return 1.0f;
    return wi[2] > 0.0f ? bp[4] : bp[5];
}

// RoughDielectric::eval (ESolidAngle, ERadiance, :317-395) into f and
// RoughDielectric::pdf (:397-469), both components enabled.  wo may lie on
// either side.
__host__ __device__ __forceinline__ float roughdielectric_eval_pdf(const float wi_[3], const float wo_[3],
                                                                   const float* bp, const float st[3], float f[3]) {
#pragma clang fp contract(off)
    f[0] = f[1] = f[2] = 0.0f;
    if (wi_[2] == 0.0f) return 0.0f;
    const double wi[3] = {wi_[0], wi_[1], wi_[2]}, wo[3] = {wo_[0], wo_[1], wo_[2]};
    const double eta = bp[4], inv_eta = bp[5], alpha = bp[6];
    const bool reflect = wi[2] * wo[2] > 0.0;
    const double e = wi[2] > 0.0 ? eta : inv_eta;
    double hs[3], H[3];
    if (reflect)
        for (int a = 0; a < 3; ++a) hs[a] = wo[a] + wi[a];
    else
        for (int a = 0; a < 3; ++a) hs[a] = wi[a] + wo[a] * e;
    normalize3(hs, H);
    // H *= signum(cosTheta(H)): the dot products below change sign together,
    // so eval's (after the flip) and pdf's (before it) agree in every bit of
    // the values used
    if (copysign(1.0, H[2]) < 0.0)
        for (int a = 0; a < 3; ++a) H[a] = -H[a];
    const double wi_h = dot3(wi, H), wo_h = dot3(wo, H);
    double cos_t;
    const double F = fresnel_dielectric_ext(wi_h, eta, &cos_t);
    const double sqrt_denom = wi_h + e * wo_h;
    const double D = beckmann_d(H, alpha);
    if (D != 0.0) {
        const double G = beckmann_g1(wi, H, alpha) * beckmann_g1(wo, H, alpha);
        if (reflect) {
            const double value = F * D * G / (4.0 * fabs(wi[2]));
            for (int ch = 0; ch < 3; ++ch) f[ch] = (float)((double)bp[1 + ch] * value);
        } else {
            const double value = ((1.0 - F) * D * G * e * e * wi_h * wo_h) / (wi[2] * sqrt_denom * sqrt_denom);
            const double factor = wi[2] > 0.0 ? inv_eta : eta;
            const double v = fabs(value * factor * factor);
            for (int ch = 0; ch < 3; ++ch) f[ch] = (float)((double)st[ch] * v);
        }
    }
    const double dwh_dwo = reflect ? 1.0 / (4.0 * wo_h) : (e * e * wo_h) / (sqrt_denom * sqrt_denom);
    double prob = beckmann_d(H, roughdielectric_sample_alpha(alpha, wi[2])) * H[2];
    prob *= reflect ? F : (1.0 - F);
    return (float)fabs(prob * dwh_dwo);
}

// RoughDielectric::sample(bRec, pdf, sample) (:560-662): wo, the weight, the
// solid-angle pdf and the crossed relative index; u2 stands where the
// reference draws bRec.sampler->next1D() for the lobe (reflection when u2 <=
// F).  false: the sample is void (weight 0, pdf 0, eta 1) -- microfacet pdf 0,
// a failed side check, cosThetaT == 0, or wi.z == 0.
__host__ __device__ __forceinline__ bool roughdielectric_sample(const float wi_[3], const float* bp,
                                                                const float st[3], float u0, float u1, float u2,
                                                                float wo_[3], float bw[3], float* pdf,
                                                                float* eta_out) {
#pragma clang fp contract(off)
    const double eta = bp[4], inv_eta = bp[5], alpha = bp[6];
    *pdf = 0.0f;
    *eta_out = 1.0f;
    bw[0] = bw[1] = bw[2] = 0.0f;
    wo_[0] = 0.0f; wo_[1] = 0.0f; wo_[2] = 1.0f;
    if (wi_[2] == 0.0f) return false;
    const double wi[3] = {wi_[0], wi_[1], wi_[2]};
    double m[3], wo[3];
    const double mpdf = beckmann_sample_all(roughdielectric_sample_alpha(alpha, wi[2]), (double)u0, (double)u1, m);
    if (mpdf == 0.0) return false;
    const double dm = dot3(wi, m);
    double cos_t;
    const double F = fresnel_dielectric_ext(dm, eta, &cos_t);
    const bool reflect = (double)u2 <= F;
    double p, dwh_dwo, scale = 1.0;
    float crossed = 1.0f;
    const float* tint;
    if (reflect) {
        p = mpdf * F;
        for (int a = 0; a < 3; ++a) wo[a] = 2.0 * dm * m[a] - wi[a];   // reflect
        for (int a = 0; a < 3; ++a) wo_[a] = (float)wo[a];
        if (wi[2] * wo[2] <= 0.0 || wo_[2] == 0.0f) return false;
        tint = bp + 1;
        dwh_dwo = 1.0 / (4.0 * dot3(wo, m));
    } else {
        p = mpdf * (1.0 - F);
        if (cos_t == 0.0) return false;
        // refract(wi, m, eta, cosThetaT) (libcore/util.cpp:767-772)
        const double er = cos_t < 0.0 ? inv_eta : eta;
        const double k = dm * er + cos_t;
        for (int a = 0; a < 3; ++a) wo[a] = m[a] * k - wi[a] * er;
        for (int a = 0; a < 3; ++a) wo_[a] = (float)wo[a];
        crossed = cos_t < 0.0 ? bp[4] : bp[5];
        if (wi[2] * wo[2] >= 0.0 || wo_[2] == 0.0f) return false;
        // the solid-angle compression of radiance across the interface
        const double factor = cos_t < 0.0 ? inv_eta : eta;
        tint = st;
        scale = factor * factor;
        const double wo_m = dot3(wo, m), ce = (double)crossed;
        const double sqrt_denom = dm + ce * wo_m;
        dwh_dwo = (ce * ce * wo_m) / (sqrt_denom * sqrt_denom);
    }
    const double g = beckmann_g1(wi, m, alpha) * beckmann_g1(wo, m, alpha);
    const double weight = fabs(beckmann_d(m, alpha) * g * dm / (mpdf * wi[2]));
    // (a transmitted weight: specularTransmittance * factor^2, then the scalar)
    for (int ch = 0; ch < 3; ++ch) bw[ch] = (float)(((double)tint[ch] * scale) * weight);
    *pdf = (float)fabs(p * dwh_dwo);
    *eta_out = crossed;
    return true;
}

}  // namespace sdmm
