// bsdf_beckmann.h -- the isotropic Beckmann microfacet distribution with
// sampleVisible = false (bsdfs/microfacet.h: eval :191-233, sampleAll :287-395,
// pdfAll :404-407, smithG1 :477-518) and the small vector helpers its users
// share, host + device, as templates on the real type T: the rough conductor
// of render.hip runs them in float (the reference's Float; its operation order
// is the one written here), the rough dielectric of bsdf_roughdielectric.h in
// double.  Arithmetic without contraction; exp / log / sin / cos as
// (T)f((double)x): math::fastexp / fastlog on Linux x86_64 (math.h:185-197)
// and the library's sincos convention.  The reference's float constants keep
// their float values at either T.
#pragma once
#include <hip/hip_runtime.h>

namespace sdmm {

constexpr float kPiF = 3.14159265358979323846f;

template <class T> __host__ __device__ __forceinline__ T real_pi();
template <> __host__ __device__ __forceinline__ float real_pi<float>() { return kPiF; }
template <> __host__ __device__ __forceinline__ double real_pi<double>() { return 3.14159265358979323846; }
__host__ __device__ __forceinline__ float real_sqrt(float x) { return sqrtf(x); }
__host__ __device__ __forceinline__ double real_sqrt(double x) { return sqrt(x); }
__host__ __device__ __forceinline__ float real_abs(float x) { return fabsf(x); }
__host__ __device__ __forceinline__ double real_abs(double x) { return fabs(x); }
__host__ __device__ __forceinline__ float real_max(float a, float b) { return fmaxf(a, b); }
__host__ __device__ __forceinline__ double real_max(double a, double b) { return fmax(a, b); }

template <class T>
__host__ __device__ __forceinline__ T dot3(const T a[3], const T b[3]) {
#pragma clang fp contract(off)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// Vector3 normalize (v * (1 / |v|), vector.h:625-627)
template <class T>
__host__ __device__ __forceinline__ void normalize3(const T v[3], T r[3]) {
#pragma clang fp contract(off)
    const T rc = T(1) / real_sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    r[0] = v[0] * rc; r[1] = v[1] * rc; r[2] = v[2] * rc;
}

// MicrofacetDistribution::eval (microfacet.h:191-233), Beckmann
template <class T>
__host__ __device__ __forceinline__ T beckmann_d(const T m[3], T alpha) {
#pragma clang fp contract(off)
    if (m[2] <= T(0)) return T(0);
    const T ct2 = m[2] * m[2];
    const T ex = ((m[0] * m[0]) / (alpha * alpha) + (m[1] * m[1]) / (alpha * alpha)) / ct2;
    T r = (T)exp((double)-ex) / (real_pi<T>() * alpha * alpha * ct2 * ct2);
    if (r * m[2] < T(1e-20f)) r = T(0);
    return r;
}

// smithG1 (microfacet.h:477-518), Beckmann's rational approximation
template <class T>
__host__ __device__ __forceinline__ T beckmann_g1(const T v[3], const T m[3], T alpha) {
#pragma clang fp contract(off)
    if (dot3(v, m) * v[2] <= T(0)) return T(0);
    const T tmp = T(1) - v[2] * v[2];
    const T tan_t = tmp <= T(0) ? T(0) : real_abs(real_sqrt(tmp) / v[2]);
    if (tan_t == T(0)) return T(1);
    const T a = T(1) / (alpha * tan_t);
    if (a >= T(1.6f)) return T(1);
    const T a2 = a * a;
    return (T(3.535f) * a + T(2.181f) * a2) / (T(1) + T(2.276f) * a + T(2.577f) * a2);
}

// sampleAll (microfacet.h:287-395), isotropic Beckmann: the microfacet normal
// m of (u0, u1) and its solid-angle density (0 below 1e-20)
template <class T>
__host__ __device__ __forceinline__ T beckmann_sample_all(T alpha, T u0, T u1, T m[3]) {
#pragma clang fp contract(off)
    const T phi = (T(2) * real_pi<T>()) * u1;
    double sd, cd;
    sincos((double)phi, &sd, &cd);
    const T sp = (T)sd, cp = (T)cd;
    const T a2 = alpha * alpha;
    const T tan2 = a2 * -(T)log((double)(T(1) - u0));
    const T ct = T(1) / real_sqrt(T(1) + tan2);
    T mpdf = (T(1) - u0) / (real_pi<T>() * alpha * alpha * ct * ct * ct);
    if (mpdf < T(1e-20f)) mpdf = T(0);
    const T st = real_sqrt(real_max(T(0), T(1) - ct * ct));
    m[0] = st * cp; m[1] = st * sp; m[2] = ct;
    return mpdf;
}

}  // namespace sdmm
