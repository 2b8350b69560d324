// film.h -- the film: a run's render passes combined by inverse variance and
// scored against a ground truth, host + device, one source.  It restates what
// the reference does after the render, scripts/combine_renders.py:167-270 (the
// per-pixel variance of a pass from its mean and mean-of-squares images, the
// three weighting heuristics, the running combination) and scripts/
// test_suite_utils.py:116-155 (MrSE, MAPE, SMAPE), in the float32 arithmetic
// numpy runs there: one rounding per operation, no contraction, np.clip and
// np.maximum keeping a NaN.  film.hip's kernels and the host film of
// film_api.cpp run the same functions, so the two agree bitwise.  No HIP
// include; under hipcc the functions are __host__ __device__.
//
// Departure: the three reductions (per-channel variance, mean pixel variance,
// the error means) are fp64 sums in the fixed order defined below, not numpy's
// float32 pairwise np.mean ("Film").
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SDMM_FILM_HD __host__ __device__ __forceinline__
#else
#define SDMM_FILM_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sdmm {

constexpr int kFilmVar = 0;       // weight: the pass's per-channel variance
constexpr int kFilmMaxVar = 1;    // weight: max(pixel variance, per-channel variance)
constexpr int kFilmUniform = 2;   // weight: 1 / spp
constexpr int64_t kFilmMaxPixels = (int64_t)1 << 26;

// ---- per pixel ---------------------------------------------------------------
// np.clip: a NaN stays a NaN (fminf / fmaxf would drop it)
SDMM_FILM_HD float film_clip(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// np.maximum: a NaN on either side is the result
SDMM_FILM_HD float film_max_nan(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// spp / (spp - 1) in double, rounded once (a Python float against a float32 array)
SDMM_FILM_HD float film_var_coef(int spp) { return (float)((double)spp / (double)(spp - 1)); }

// combine_renders.py:213-219.  img and sqr are already the pass's means; the
// reference divides them by spp again, and its weights depend on that.
SDMM_FILM_HD float film_variance(float img, float sqr, float fspp, float coef) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float m = img / fspp;
    const float s = sqr / fspp;
    const float mm = m * m;
    const float d = s - mm;
    const float v = coef * d;
    return film_clip(v, 0.0f, 2000.0f);
}

// :232-242, the weight of one element: pcv is the pass's per-channel variance
// as float32, wu = float32(1.0 / spp); var is read in kFilmMaxVar only.
SDMM_FILM_HD float film_weight(int mode, float var, float pcv, float wu) {
    return mode == kFilmUniform ? wu : (mode == kFilmMaxVar ? film_max_nan(var, pcv) : pcv);
}
SDMM_FILM_HD float film_uniform_weight(int spp) { return (float)(1.0 / (double)spp); }

// final (+)= img / w and recip (+)= 1 / w; the first included pass assigns
SDMM_FILM_HD float film_accumulate(bool first, float acc, float img, float w) {
    const float t = img / w;
    return first ? t : acc + t;
}
SDMM_FILM_HD float film_recip(bool first, float acc, float w) {
    const float t = 1.0f / w;
    return first ? t : acc + t;
}
SDMM_FILM_HD float film_resolve(float final_, float recip) { return final_ / recip; }

// test_suite_utils.py:148-155, the three terms of one element (before rgb_mean
// and aggregate): t[0] MrSE on values clipped to [0, 1], t[1] MAPE, t[2] SMAPE
SDMM_FILM_HD void film_error_terms(float a, float g, float t[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float ac = film_clip(a, 0.0f, 1.0f), gc = film_clip(g, 0.0f, 1.0f);
    const float dc = ac - gc;
    const float gg = gc * gc;
    t[0] = (dc * dc) / (0.01f + gg);
    const float e = fabsf(a - g);
    const float den = 0.01f + g;
    t[1] = e / den;
    t[2] = (2.0f * e) / (den + a);
}

// The combined estimate's divisor, wherever the mode keeps it.
struct FilmRecip {
    const float* plane;   // kFilmMaxVar: [3][npix]
    const float* ch;      // kFilmVar: [3]
    float uniform;        // kFilmUniform: the double sum rounded to float32
    int mode;
};
SDMM_FILM_HD float film_recip_at(const FilmRecip& r, int ch, int64_t npix, int64_t i) {
    return r.mode == kFilmUniform ? r.uniform : (r.mode == kFilmMaxVar ? r.plane[(int64_t)ch * npix + i] : r.ch[ch]);
}

// One pass as the kernels and the host loops see it: planes [3][npix].
struct FilmPassDev {
    const float* img;
    const float* sqr;
    int64_t npix;
    float fspp;   // float32(spp)
    float coef;   // film_var_coef(spp)
};

// Where a reduction's means go.  errors = 0: rec[0..2] = pcv, rec[3] = the mean
// pixel variance, copied to hist[0..3]; recip3 (kFilmVar, an included pass,
// else NULL) takes recip[ch] (+)= 1 / float32(pcv[ch]).  errors = 1: rec[0..2]
// = MrSE, MAPE, SMAPE.
struct FilmFinishDev {
    double* rec;
    double* hist;
    float* recip3;
    int64_t npix;
    int first;
    int errors;
};

// ---- the reduction's order ---------------------------------------------------
// A sum of n values (as doubles) is taken in levels.  One level turns n values
// into ceil(n / 256): chunk k covers values [256 k, 256 k + 256), a value past
// n counting as +0.0; inside a chunk, lane l of 64 first adds its four
// consecutive values as (v0 + v1) + (v2 + v3) (film_quad), then the 64 lane
// sums go through the tree q[i] += q[i + s] for i < s, s = 32, 16, 8, 4, 2, 1.
// Levels repeat until one value is left.  The first level's values are one
// channel plane's pixels, so a chunk never crosses channels; the per-channel
// sums S[0..2] then give pcv[ch] = S[ch] / npix and the all-channel mean
// ((S[0] + S[1]) + S[2]) / (3 npix).  Nothing here depends on a grid, a block
// size or the device: the kernels run one wave per chunk and take the tree with
// lane shuffles, the host loop below runs the identical additions.
constexpr int kFilmChunk = 256;
constexpr int kFilmLanes = 64;
constexpr int kFilmQuad = kFilmChunk / kFilmLanes;
static_assert(kFilmQuad == 4, "film_quad adds four values per lane");

SDMM_FILM_HD double film_quad(double v0, double v1, double v2, double v3) { return (v0 + v1) + (v2 + v3); }
SDMM_FILM_HD int64_t film_chunks(int64_t n) { return (n + kFilmChunk - 1) / kFilmChunk; }
SDMM_FILM_HD double film_mean(double s, int64_t npix) { return s / (double)npix; }
SDMM_FILM_HD double film_mean3(double s0, double s1, double s2, int64_t npix) {
    return ((s0 + s1) + s2) / (3.0 * (double)npix);
}

// the 64-lane tree on the host (the device takes it with __shfl_down)
inline double film_tree_host(double q[kFilmLanes]) {
    for (int s = kFilmLanes / 2; s >= 1; s >>= 1)
        for (int i = 0; i < s; ++i) q[i] += q[i + s];
    return q[0];
}

// one chunk on the host: value(i) for i in [base, base + 256), +0.0 past n
template <class F>
inline double film_chunk_host(int64_t base, int64_t n, F value) {
    double q[kFilmLanes];
    for (int l = 0; l < kFilmLanes; ++l) {
        double v[kFilmQuad];
        for (int j = 0; j < kFilmQuad; ++j) {
            const int64_t i = base + (int64_t)l * kFilmQuad + j;
            v[j] = i < n ? value(i) : 0.0;
        }
        q[l] = film_quad(v[0], v[1], v[2], v[3]);
    }
    return film_tree_host(q);
}

// the levels after the first on the host: x[0..n) -> one value (x is overwritten)
inline double film_reduce_host(double* x, int64_t n) {
    while (n > 1) {
        const int64_t m = film_chunks(n);
        for (int64_t k = 0; k < m; ++k) {
            const double s = film_chunk_host(k * kFilmChunk, n, [&](int64_t i) { return x[i]; });
            x[k] = s;   // chunk k's inputs start at 256 k >= k: already consumed
        }
        n = m;
    }
    return x[0];
}

}  // namespace sdmm
