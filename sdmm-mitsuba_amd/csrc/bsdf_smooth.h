// bsdf_smooth.h -- the two delta-only BSDFs, the smooth dielectric (mitsuba/
// src/bsdfs/dielectric.cpp: eval :228-253, pdf :255-275, sample(bRec, pdf,
// sample) :277-333; ERadiance, both components) and the smooth conductor
// (bsdfs/conductor.cpp: eval :223-237, pdf :239-252, sample :270-285), in the
// local shading frame, host + device: the device Li's loop head samples them
// (a pure-delta bounce: no guide query, no saved vertex, sdmm_proc.cpp:297-302,
// :764), and the host ABI sdmm_bsdf_smooth_host and the batch kernel behind
// sdmm_bsdf_smooth_device run the same code (tests/test_bsdf_smooth.py checks
// it against the formulas in float64).
//
// bp: the BSDF's 8 bsdf_params floats.  Smooth dielectric (kind 5): [1..3]
// specularReflectance, [4] eta = intIOR / extIOR, [5] 1 / eta; st: its
// specularTransmittance (the BSDF's `reflectance` row).  wi.z < 0 is a hit
// from inside: the interface is two-sided.  wi.z == 0 samples and evaluates to
// 0.  Smooth conductor (kind 6): [1..3] specularReflectance, [4] eta, [5] k (a
// gray conductor, as the rough one); one-sided, wi.z <= 0 gives 0; st unused.
//
// Inputs and outputs are floats; the arithmetic between them is double,
// without contraction (as bsdf_roughdielectric.h: cosThetaT cancels near the
// critical angle, and the host and the device then round the same double
// once).  fresnel_conductor is the one copy of fresnelConductorExact: the
// rough conductor of render.hip runs it in float, the smooth one in double.
#pragma once
#include <hip/hip_runtime.h>

#include "bsdf_roughdielectric.h"
#include "render_device.h"

namespace sdmm {

constexpr float kDeltaEpsilon = 1e-3f;     // Mitsuba's DeltaEpsilon (core/constants.h)

namespace detail {
// sqrt / fmax of fresnel_conductor's real type (the float ones as render.hip called them)
__host__ __device__ __forceinline__ float fc_sqrt(float x) { return sqrtf(x); }
__host__ __device__ __forceinline__ double fc_sqrt(double x) { return sqrt(x); }
__host__ __device__ __forceinline__ float fc_max(float a, float b) { return fmaxf(a, b); }
__host__ __device__ __forceinline__ double fc_max(double a, double b) { return fmax(a, b); }
}  // namespace detail

// fresnelConductorExact (libcore/util.cpp:739-761, the Spectrum form) for a
// gray conductor: the unpolarised reflectance at cos(theta_i) for the index
// eta + i k
template <typename T>
__host__ __device__ __forceinline__ T fresnel_conductor(T ci, T eta, T k) {
#pragma clang fp contract(off)
    const T ci2 = ci * ci, si2 = T(1) - ci2, si4 = si2 * si2;
    const T t1 = eta * eta - k * k - si2;
    const T a2pb2 = detail::fc_sqrt(detail::fc_max(T(0), t1 * t1 + k * k * eta * eta * T(4)));
    const T a = detail::fc_sqrt(detail::fc_max(T(0), (a2pb2 + t1) * T(0.5)));
    const T term1 = a2pb2 + ci2, term2 = a * (T(2) * ci);
    const T rs2 = (term1 - term2) / (term1 + term2);
    const T term3 = a2pb2 * ci2 + si4, term4 = term2 * si2;
    const T rp2 = rs2 * (term3 - term4) / (term3 + term4);
    return T(0.5) * (rp2 + rs2);
}

// a kind-5 or kind-6 parameter row
__host__ __device__ __forceinline__ bool is_smooth_kind(float kind) {
    return kind == (float)kBsdfSmoothDielectric || kind == (float)kBsdfSmoothConductor;
}

// sample(bRec, pdf, sample) of either BSDF, by bp[0]: wo, the weight, the
// discrete pdf and bRec.eta; u0 is sample.x (reflection when u0 <= F: at a
// total internal reflection F = 1, so the sample always reflects).  false: the
// weight is 0 (wi.z == 0, the conductor's back side, or a zero reflectance /
// transmittance of the chosen lobe); pdf 0, eta 1 and wo = +z for the first
// two, the chosen lobe's otherwise.
__host__ __device__ __forceinline__ bool smooth_sample(const float wi[3], const float* bp, const float st[3],
                                                       float u0, float wo[3], float bw[3], float* pdf,
                                                       float* eta_out) {
#pragma clang fp contract(off)
    *pdf = 0.0f;
    *eta_out = 1.0f;
    bw[0] = bw[1] = bw[2] = 0.0f;
    wo[0] = 0.0f; wo[1] = 0.0f; wo[2] = 1.0f;
    if (bp[0] == (float)kBsdfSmoothConductor) {
        // SmoothConductor::sample (conductor.cpp:270-285)
        if (wi[2] <= 0.0f) return false;
        wo[0] = -wi[0]; wo[1] = -wi[1]; wo[2] = wi[2];
        const double fr = fresnel_conductor<double>((double)wi[2], (double)bp[4], (double)bp[5]);
        for (int ch = 0; ch < 3; ++ch) bw[ch] = (float)((double)bp[1 + ch] * fr);
        *pdf = 1.0f;
        return bw[0] != 0.0f || bw[1] != 0.0f || bw[2] != 0.0f;
    }
    // SmoothDielectric::sample (dielectric.cpp:277-308)
    if (wi[2] == 0.0f) return false;
    const double eta = bp[4], inv_eta = bp[5];
    double cos_t;
    const double F = fresnel_dielectric_ext((double)wi[2], eta, &cos_t);
    if ((double)u0 <= F) {
        wo[0] = -wi[0]; wo[1] = -wi[1]; wo[2] = wi[2];
        for (int ch = 0; ch < 3; ++ch) bw[ch] = bp[1 + ch];
        *pdf = (float)F;
    } else {
        // refract(wi, cosThetaT) (:223-226); the solid-angle compression of
        // radiance across the interface, factor^2
        const double factor = cos_t < 0.0 ? inv_eta : eta;
        wo[0] = (float)(-factor * (double)wi[0]);
        wo[1] = (float)(-factor * (double)wi[1]);
        wo[2] = (float)cos_t;
        for (int ch = 0; ch < 3; ++ch) bw[ch] = (float)((double)st[ch] * (factor * factor));
        *pdf = (float)(1.0 - F);
        *eta_out = cos_t < 0.0 ? bp[4] : bp[5];
    }
    return bw[0] != 0.0f || bw[1] != 0.0f || bw[2] != 0.0f;
}

// eval and pdf (EDiscrete) of a given wo: the lobe's value (reflectance * F,
// transmittance * factor^2 * (1 - F), reflectance * F_conductor) and its
// discrete probability where wo lies within DeltaEpsilon of the lobe's
// direction (|dot - 1| <= 1e-3), 0 elsewhere; *eta_out what sample would have
// set for that lobe.
__host__ __device__ __forceinline__ float smooth_eval_pdf(const float wi_[3], const float wo_[3], const float* bp,
                                                          const float st[3], float f[3], float* eta_out) {
#pragma clang fp contract(off)
    f[0] = f[1] = f[2] = 0.0f;
    *eta_out = 1.0f;
    const double wi[3] = {wi_[0], wi_[1], wi_[2]}, wo[3] = {wo_[0], wo_[1], wo_[2]};
    const double refl_dot = -wi[0] * wo[0] - wi[1] * wo[1] + wi[2] * wo[2];   // dot(reflect(wi), wo)
    if (bp[0] == (float)kBsdfSmoothConductor) {
        if (wi_[2] <= 0.0f || wo_[2] <= 0.0f || fabs(refl_dot - 1.0) > (double)kDeltaEpsilon) return 0.0f;
        const double fr = fresnel_conductor<double>(wi[2], (double)bp[4], (double)bp[5]);
        for (int ch = 0; ch < 3; ++ch) f[ch] = (float)((double)bp[1 + ch] * fr);
        return 1.0f;
    }
    if (wi_[2] == 0.0f) return 0.0f;
    const double eta = bp[4], inv_eta = bp[5];
    double cos_t;
    const double F = fresnel_dielectric_ext(wi[2], eta, &cos_t);
    if (wi[2] * wo[2] >= 0.0) {
        if (fabs(refl_dot - 1.0) > (double)kDeltaEpsilon) return 0.0f;
        for (int ch = 0; ch < 3; ++ch) f[ch] = (float)((double)bp[1 + ch] * F);
        return (float)F;
    }
    const double factor = cos_t < 0.0 ? inv_eta : eta;
    *eta_out = cos_t < 0.0 ? bp[4] : bp[5];
    const double refr_dot = (-factor * wi[0]) * wo[0] + (-factor * wi[1]) * wo[1] + cos_t * wo[2];
    if (fabs(refr_dot - 1.0) > (double)kDeltaEpsilon) return 0.0f;
    for (int ch = 0; ch < 3; ++ch) f[ch] = (float)(((double)st[ch] * (factor * factor)) * (1.0 - F));
    return (float)(1.0 - F);
}

}  // namespace sdmm
