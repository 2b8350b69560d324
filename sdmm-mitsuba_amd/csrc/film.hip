// film.hip -- the device film's kernels (gfx950): the per-pass variance with
// its fp64 reduction, the inverse-variance accumulate, the resolve and the
// error means.  The arithmetic and the reduction's order are film.h's, shared
// with the host film (film_api.cpp); this file only maps them onto waves.
//
// All four are bandwidth kernels over [3][npix] float planes: 16-byte loads
// and stores where every plane is 16-byte aligned and npix is a multiple of 4
// (VEC), scalar accesses otherwise; one pass over the data per kernel.  The
// reducing kernels run one wave per 256-value chunk (film.h): a lane's four
// values, then the 64-lane tree by __shfl_down, lane 0 storing the chunk's
// partial -- no floating-point atomics, and a grid-stride loop over chunks, so
// the result does not depend on the grid.  film_finish_kernel takes the levels
// after the first in one block and writes the means to the film's device
// record, from where the accumulate kernel reads the pass's per-channel
// variance: sdmm_film_add_pass needs no host synchronisation.
#include <hip/hip_runtime.h>

#include "film.h"
#include "render_launch.h"

namespace sdmm {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kFilmLanes;
constexpr int kReduceBlocksMax = 8192;   // one chunk per wave up to 8.4 M values; a 1920 x 1080 pass has 6.2 M
constexpr int kStreamBlocksMax = 1024;
constexpr int kFinishBlock = 1024;

__device__ __forceinline__ double wave_tree(double v) {
#pragma unroll
    for (int s = kFilmLanes / 2; s >= 1; s >>= 1) v += __shfl_down(v, s, kFilmLanes);
    return v;   // lane 0: film_tree_host's q[0]
}

// four consecutive values of a plane from `base`; past n: 0 (never summed)
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ plane, int64_t base, int64_t n, float v[4]) {
    if constexpr (VEC) {
        if (base < n) {   // n is a multiple of 4: the quad is inside
            const float4 t = *reinterpret_cast<const float4*>(plane + base);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            v[0] = v[1] = v[2] = v[3] = 0.0f;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = base + j < n ? plane[base + j] : 0.0f;
    }
}
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ plane, int64_t base, int64_t n, const float v[4]) {
    if constexpr (VEC) {
        if (base < n) *reinterpret_cast<float4*>(plane + base) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (base + j < n) plane[base + j] = v[j];
    }
}

// level 1 of the variance sums: partials[ch * n1 + k], chunk k of channel ch
template <bool VEC>
__global__ void __launch_bounds__(kBlock)
film_var_reduce_kernel(FilmPassDev p, int64_t n1, double* __restrict__ partials) {
    const int lane = threadIdx.x & (kFilmLanes - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t cid = wave; cid < 3 * n1; cid += nwaves) {
        const int64_t ch = cid / n1, k = cid - ch * n1;
        const int64_t base = k * kFilmChunk + (int64_t)lane * kFilmQuad;
        float a[4], s[4];
        load4<VEC>(p.img + ch * p.npix, base, p.npix, a);
        load4<VEC>(p.sqr + ch * p.npix, base, p.npix, s);
        double d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            d[j] = base + j < p.npix ? (double)film_variance(a[j], s[j], p.fspp, p.coef) : 0.0;
        const double v = wave_tree(film_quad(d[0], d[1], d[2], d[3]));
        if (lane == 0) partials[cid] = v;
    }
}

// level 1 of the error sums: partials[(metric * 3 + ch) * n1 + k]
template <bool VEC>
__global__ void __launch_bounds__(kBlock)
film_err_reduce_kernel(const float* __restrict__ image, const float* __restrict__ final_, FilmRecip r,
                       const float* __restrict__ truth, int64_t npix, int64_t n1, double* __restrict__ partials) {
    const int lane = threadIdx.x & (kFilmLanes - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t cid = wave; cid < 3 * n1; cid += nwaves) {
        const int64_t ch = cid / n1, k = cid - ch * n1;
        const int64_t base = k * kFilmChunk + (int64_t)lane * kFilmQuad;
        float a[4], g[4];
        load4<VEC>(truth + ch * npix, base, npix, g);
        if (image) {
            load4<VEC>(image + ch * npix, base, npix, a);
        } else {
            load4<VEC>(final_ + ch * npix, base, npix, a);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (base + j < npix) a[j] = film_resolve(a[j], film_recip_at(r, (int)ch, npix, base + j));
        }
        double d[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float t[3];
            film_error_terms(a[j], g[j], t);
            const bool in = base + j < npix;
#pragma unroll
            for (int m = 0; m < 3; ++m) d[m][j] = in ? (double)t[m] : 0.0;
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const double v = wave_tree(film_quad(d[m][0], d[m][1], d[m][2], d[m][3]));
            if (lane == 0) partials[((int64_t)m * 3 + ch) * n1 + k] = v;
        }
    }
}

// The levels after the first, one block: rows x n values in p0 (row stride n)
// -> rows sums, ping-pong between p0 and p1; then the means.  __syncthreads
// orders a level's stores before the next level's loads (one workgroup).
__global__ void __launch_bounds__(kFinishBlock)
film_finish_kernel(double* p0, double* p1, int rows, int64_t n, FilmFinishDev f) {
    const int lane = threadIdx.x & (kFilmLanes - 1);
    const int wave = threadIdx.x >> 6;
    double* src = p0;
    double* dst = p1;
    while (n > 1) {
        const int64_t m = film_chunks(n);
        for (int64_t item = wave; item < (int64_t)rows * m; item += kFinishBlock / kFilmLanes) {
            const int64_t row = item / m, k = item - row * m;
            const double* x = src + row * n;
            const int64_t base = k * kFilmChunk + (int64_t)lane * kFilmQuad;
            double d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = base + j < n ? x[base + j] : 0.0;
            const double v = wave_tree(film_quad(d[0], d[1], d[2], d[3]));
            if (lane == 0) dst[item] = v;
        }
        __syncthreads();
        double* t = src;
        src = dst;
        dst = t;
        n = m;
    }
    if (threadIdx.x != 0) return;
    if (f.errors) {
        for (int m = 0; m < 3; ++m) f.rec[m] = film_mean3(src[3 * m], src[3 * m + 1], src[3 * m + 2], f.npix);
        return;
    }
    double out[4];
    for (int c = 0; c < 3; ++c) out[c] = film_mean(src[c], f.npix);
    out[3] = film_mean3(src[0], src[1], src[2], f.npix);
    for (int i = 0; i < 4; ++i) {
        f.rec[i] = out[i];
        f.hist[i] = out[i];
    }
    if (f.recip3)   // kFilmVar, an included pass: recip[ch] (+)= 1 / w
        for (int c = 0; c < 3; ++c) f.recip3[c] = film_recip(f.first != 0, f.recip3[c], (float)out[c]);
}

// final (+)= img / w; kFilmMaxVar: the pixel's variance again from img and
// sqr, and its recip plane.  grid.y: the channel; a thread: 4 consecutive pixels.
template <bool VEC>
__global__ void __launch_bounds__(kBlock)
film_accum_kernel(FilmPassDev p, int mode, const double* __restrict__ rec, float wu, int first,
                  float* __restrict__ final_, float* __restrict__ recip_plane) {
    const int ch = blockIdx.y;
    const float pcv = mode == kFilmUniform ? 0.0f : (float)rec[ch];
    const int64_t nq = (p.npix + 3) / 4, off = (int64_t)ch * p.npix;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += (int64_t)gridDim.x * kBlock) {
        const int64_t base = q * 4;
        float a[4], s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, rc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        load4<VEC>(p.img + off, base, p.npix, a);
        if (mode == kFilmMaxVar) load4<VEC>(p.sqr + off, base, p.npix, s);
        if (!first) {
            load4<VEC>(final_ + off, base, p.npix, acc);
            if (mode == kFilmMaxVar) load4<VEC>(recip_plane + off, base, p.npix, rc);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float var = mode == kFilmMaxVar ? film_variance(a[j], s[j], p.fspp, p.coef) : 0.0f;
            const float w = film_weight(mode, var, pcv, wu);
            acc[j] = film_accumulate(first != 0, acc[j], a[j], w);
            rc[j] = film_recip(first != 0, rc[j], w);
        }
        store4<VEC>(final_ + off, base, p.npix, acc);
        if (mode == kFilmMaxVar) store4<VEC>(recip_plane + off, base, p.npix, rc);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(kBlock)
film_resolve_kernel(const float* __restrict__ final_, FilmRecip r, int64_t npix, float* __restrict__ out) {
    const int ch = blockIdx.y;
    const int64_t nq = (npix + 3) / 4, off = (int64_t)ch * npix;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += (int64_t)gridDim.x * kBlock) {
        const int64_t base = q * 4;
        float a[4], rc[4];
        load4<VEC>(final_ + off, base, npix, a);
        if (r.mode == kFilmMaxVar) {
            load4<VEC>(r.plane + off, base, npix, rc);
        } else {
            const float v = r.mode == kFilmUniform ? r.uniform : r.ch[ch];
            rc[0] = rc[1] = rc[2] = rc[3] = v;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = film_resolve(a[j], rc[j]);
        store4<VEC>(out + off, base, npix, a);
    }
}

// the clipped per-pixel variance into caller planes (sdmm_film_variance)
template <bool VEC>
__global__ void __launch_bounds__(kBlock)
film_variance_kernel(FilmPassDev p, float* __restrict__ out) {
    const int ch = blockIdx.y;
    const int64_t nq = (p.npix + 3) / 4, off = (int64_t)ch * p.npix;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += (int64_t)gridDim.x * kBlock) {
        const int64_t base = q * 4;
        float a[4], s[4];
        load4<VEC>(p.img + off, base, p.npix, a);
        load4<VEC>(p.sqr + off, base, p.npix, s);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = film_variance(a[j], s[j], p.fspp, p.coef);
        store4<VEC>(out + off, base, p.npix, a);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

dim3 reduce_grid(int64_t n1) {
    const int64_t b = (3 * n1 + kWavesPerBlock - 1) / kWavesPerBlock;
    return dim3((unsigned)(b < kReduceBlocksMax ? b : kReduceBlocksMax));
}
dim3 stream_grid(int64_t npix) {
    const int64_t b = ((npix + 3) / 4 + kBlock - 1) / kBlock;
    return dim3((unsigned)(b < kStreamBlocksMax ? b : kStreamBlocksMax), 3);
}

}  // namespace

size_t film_partials_doubles(int64_t npix, int which) {
    const int64_t n1 = film_chunks(npix);
    return (size_t)(9 * (which == 0 ? n1 : film_chunks(n1)));
}

hipError_t launch_film_var_reduce(const FilmPassDev& p, double* p0, double* p1, const FilmFinishDev& f,
                                  hipStream_t st) {
    const int64_t n1 = film_chunks(p.npix);
    if (aligned16(p.img) && aligned16(p.sqr) && p.npix % 4 == 0)
        hipLaunchKernelGGL(film_var_reduce_kernel<true>, reduce_grid(n1), dim3(kBlock), 0, st, p, n1, p0);
    else
        hipLaunchKernelGGL(film_var_reduce_kernel<false>, reduce_grid(n1), dim3(kBlock), 0, st, p, n1, p0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(film_finish_kernel, dim3(1), dim3(kFinishBlock), 0, st, p0, p1, 3, n1, f);
    return hipGetLastError();
}

hipError_t launch_film_accumulate(const FilmPassDev& p, int mode, const double* rec, float wu, int first,
                                  float* final_, float* recip_plane, hipStream_t st) {
    const bool vec = aligned16(p.img) && aligned16(p.sqr) && aligned16(final_) && aligned16(recip_plane) &&
                     p.npix % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(film_accum_kernel<true>, stream_grid(p.npix), dim3(kBlock), 0, st, p, mode, rec, wu, first,
                           final_, recip_plane);
    else
        hipLaunchKernelGGL(film_accum_kernel<false>, stream_grid(p.npix), dim3(kBlock), 0, st, p, mode, rec, wu,
                           first, final_, recip_plane);
    return hipGetLastError();
}

hipError_t launch_film_resolve(const float* final_, const FilmRecip& r, int64_t npix, float* out, hipStream_t st) {
    if (aligned16(final_) && aligned16(r.plane) && aligned16(out) && npix % 4 == 0)
        hipLaunchKernelGGL(film_resolve_kernel<true>, stream_grid(npix), dim3(kBlock), 0, st, final_, r, npix, out);
    else
        hipLaunchKernelGGL(film_resolve_kernel<false>, stream_grid(npix), dim3(kBlock), 0, st, final_, r, npix, out);
    return hipGetLastError();
}

hipError_t launch_film_errors(const float* image, const float* final_, const FilmRecip& r, const float* truth,
                              int64_t npix, double* p0, double* p1, const FilmFinishDev& f, hipStream_t st) {
    const int64_t n1 = film_chunks(npix);
    const bool vec = aligned16(image) && aligned16(final_) && aligned16(r.plane) && aligned16(truth) && npix % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(film_err_reduce_kernel<true>, reduce_grid(n1), dim3(kBlock), 0, st, image, final_, r, truth,
                           npix, n1, p0);
    else
        hipLaunchKernelGGL(film_err_reduce_kernel<false>, reduce_grid(n1), dim3(kBlock), 0, st, image, final_, r,
                           truth, npix, n1, p0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(film_finish_kernel, dim3(1), dim3(kFinishBlock), 0, st, p0, p1, 9, n1, f);
    return hipGetLastError();
}

hipError_t launch_film_variance(const FilmPassDev& p, float* out, hipStream_t st) {
    if (aligned16(p.img) && aligned16(p.sqr) && aligned16(out) && p.npix % 4 == 0)
        hipLaunchKernelGGL(film_variance_kernel<true>, stream_grid(p.npix), dim3(kBlock), 0, st, p, out);
    else
        hipLaunchKernelGGL(film_variance_kernel<false>, stream_grid(p.npix), dim3(kBlock), 0, st, p, out);
    return hipGetLastError();
}

}  // namespace sdmm
