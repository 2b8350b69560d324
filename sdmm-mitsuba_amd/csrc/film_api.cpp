// film_api.cpp -- sdmm_film_* of include/sdmm_gpu.h: the device film over
// film.hip's kernels and the host film, the same film.h code in plain loops
// (no HIP call: it runs without a GPU, and is what the device film is tested
// against bitwise).  Reference: scripts/combine_renders.py:167-270 and
// scripts/test_suite_utils.py:116-155.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/sdmm_gpu.h"
#include "film.h"
#include "host_xfer.h"
#include "render_launch.h"

using namespace sdmm;

namespace {

int fail(int code, const std::string& m) { return sdmm_detail::set_error(code, m.c_str()); }

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(SDMM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

constexpr int kHistBlock = 256;   // passes per device block of the statistics history

struct Pass {
    int iteration, spp, included;
    double v[4];   // pcv[0..2], mean pixel variance
};

}  // namespace

struct sdmm_film {
    int width = 0, height = 0, mode = 0, first_iteration = 0, device = -1;
    int64_t npix = 0;
    int n_included = 0;
    double recip_uniform = 0.0;   // kFilmUniform: combine_renders.py's Python float
    std::vector<Pass> passes;
    // host film
    std::vector<float> final_h, recip_plane_h;
    float recip3_h[3] = {0.0f, 0.0f, 0.0f};
    std::vector<double> part_h;
    // device film
    float* final_d = nullptr;
    float* recip_plane_d = nullptr;
    double* small_d = nullptr;    // rec[4] (the last pass), err[3], then float recip3[3] at +8 doubles
    double* p0 = nullptr;
    double* p1 = nullptr;
    std::vector<double*> hist_d;  // kHistBlock x 4 doubles each
    size_t fetched = 0;           // passes whose statistics are on the host
    hipStream_t last_stream = nullptr;

    float* recip3_d() const { return reinterpret_cast<float*>(small_d + 8); }
    FilmRecip recip() const {
        if (device < 0) return FilmRecip{recip_plane_h.data(), recip3_h, (float)recip_uniform, mode};
        return FilmRecip{recip_plane_d, recip3_d(), (float)recip_uniform, mode};
    }
};

namespace {

void free_device(sdmm_film* f) {
    if (f->device < 0) return;
    (void)hipSetDevice(f->device);
    (void)hipStreamSynchronize(f->last_stream);
    for (double* h : f->hist_d) (void)hipFree(h);
    (void)hipFree(f->final_d);
    (void)hipFree(f->recip_plane_d);
    (void)hipFree(f->small_d);
    (void)hipFree(f->p0);
    (void)hipFree(f->p1);
}

// device -> host through the calling thread's bounce buffer; synchronises st
int read_back(void* dst, const void* src, size_t bytes, hipStream_t st) {
    char* b = nullptr;
    HIP_TRY(sdmm_detail::bounce_buf(bytes, &b));
    HIP_TRY(hipMemcpyAsync(b, src, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(dst, b, bytes);
    return SDMM_OK;
}

// the statistics of the passes still in flight
int fetch_history(sdmm_film* f) {
    if (f->device < 0 || f->fetched == f->passes.size()) return SDMM_OK;
    HIP_TRY(hipSetDevice(f->device));
    while (f->fetched < f->passes.size()) {
        const size_t blk = f->fetched / kHistBlock, at = f->fetched % kHistBlock;
        size_t n = f->passes.size() - f->fetched;
        if (n > kHistBlock - at) n = kHistBlock - at;
        std::vector<double> tmp(4 * n);
        const int rc = read_back(tmp.data(), f->hist_d[blk] + 4 * at, sizeof(double) * 4 * n, f->last_stream);
        if (rc) return rc;
        for (size_t i = 0; i < n; ++i) std::memcpy(f->passes[f->fetched + i].v, &tmp[4 * i], sizeof(double) * 4);
        f->fetched += n;
    }
    return SDMM_OK;
}

void fill_stats(const Pass& p, sdmm_film_stats* out) {
    for (int c = 0; c < 3; ++c) out->pcv[c] = p.v[c];
    out->mean_pixel_variance = p.v[3];
    out->included = p.included;
}

FilmPassDev pass_of(const sdmm_film* f, const float* image, const float* image_sqr, int spp) {
    return FilmPassDev{image, image_sqr, f->npix, (float)spp, film_var_coef(spp)};
}

// the host film's variance sums: film.h's order, chunk by chunk
void host_var_reduce(sdmm_film* f, const FilmPassDev& p, double v[4]) {
    const int64_t n1 = film_chunks(p.npix);
    f->part_h.resize((size_t)(9 * n1));
    double s[3];
    for (int ch = 0; ch < 3; ++ch) {
        const float* img = p.img + (int64_t)ch * p.npix;
        const float* sqr = p.sqr + (int64_t)ch * p.npix;
        double* part = f->part_h.data() + (int64_t)ch * n1;
        for (int64_t k = 0; k < n1; ++k)
            part[k] = film_chunk_host(k * kFilmChunk, p.npix, [&](int64_t i) {
                return (double)film_variance(img[i], sqr[i], p.fspp, p.coef);
            });
        s[ch] = film_reduce_host(part, n1);
    }
    for (int ch = 0; ch < 3; ++ch) v[ch] = film_mean(s[ch], p.npix);
    v[3] = film_mean3(s[0], s[1], s[2], p.npix);
}

void host_accumulate(sdmm_film* f, const FilmPassDev& p, const double pcv[3], float wu, bool first) {
    for (int ch = 0; ch < 3; ++ch) {
        const float w_ch = (float)pcv[ch];
        const int64_t off = (int64_t)ch * p.npix;
        for (int64_t i = 0; i < p.npix; ++i) {
            const float var =
                f->mode == kFilmMaxVar ? film_variance(p.img[off + i], p.sqr[off + i], p.fspp, p.coef) : 0.0f;
            const float w = film_weight(f->mode, var, w_ch, wu);
            f->final_h[off + i] = film_accumulate(first, f->final_h[off + i], p.img[off + i], w);
            if (f->mode == kFilmMaxVar) f->recip_plane_h[off + i] = film_recip(first, f->recip_plane_h[off + i], w);
        }
        if (f->mode == kFilmVar) f->recip3_h[ch] = film_recip(first, f->recip3_h[ch], w_ch);
    }
}

void host_errors(sdmm_film* f, const float* image, const float* truth, double out[3]) {
    const int64_t npix = f->npix, n1 = film_chunks(npix);
    const FilmRecip r = f->recip();
    f->part_h.resize((size_t)(9 * n1));
    double s[9];
    for (int m = 0; m < 3; ++m)
        for (int ch = 0; ch < 3; ++ch) {
            const int64_t off = (int64_t)ch * npix;
            double* part = f->part_h.data() + (int64_t)(m * 3 + ch) * n1;
            for (int64_t k = 0; k < n1; ++k)
                part[k] = film_chunk_host(k * kFilmChunk, npix, [&](int64_t i) {
                    const float a = image ? image[off + i]
                                          : film_resolve(f->final_h[off + i], film_recip_at(r, ch, npix, i));
                    float t[3];
                    film_error_terms(a, truth[off + i], t);
                    return (double)t[m];
                });
            s[m * 3 + ch] = film_reduce_host(part, n1);
        }
    for (int m = 0; m < 3; ++m) out[m] = film_mean3(s[3 * m], s[3 * m + 1], s[3 * m + 2], npix);
}

}  // namespace

extern "C" {

int sdmm_film_create(int width, int height, int mode, int first_iteration, int device, sdmm_film** out) {
    if (!out) return fail(SDMM_E_INVALID, "sdmm_film_create: NULL out");
    *out = nullptr;
    if (width < 1 || height < 1) return fail(SDMM_E_INVALID, "sdmm_film_create: width or height < 1");
    if ((int64_t)width * height > kFilmMaxPixels)
        return fail(SDMM_E_INVALID, "sdmm_film_create: more than 2^26 pixels");
    if (mode != kFilmVar && mode != kFilmMaxVar && mode != kFilmUniform)
        return fail(SDMM_E_INVALID, "sdmm_film_create: unknown mode (0 var, 1 max_var, 2 uniform)");
    if (first_iteration < 0) return fail(SDMM_E_INVALID, "sdmm_film_create: first_iteration < 0");
    if (device < -1) return fail(SDMM_E_INVALID, "sdmm_film_create: device < -1 (-1: a host film)");
    sdmm_film* f = new (std::nothrow) sdmm_film;
    if (!f) return fail(SDMM_E_NOMEM, "out of host memory");
    f->width = width;
    f->height = height;
    f->mode = mode;
    f->first_iteration = first_iteration;
    f->device = device;
    f->npix = (int64_t)width * height;
    const size_t n3 = (size_t)(3 * f->npix);
    if (device < 0) {
        try {
            f->final_h.assign(n3, 0.0f);
            if (mode == kFilmMaxVar) f->recip_plane_h.assign(n3, 0.0f);
        } catch (const std::bad_alloc&) {
            delete f;
            return fail(SDMM_E_NOMEM, "out of host memory");
        }
        *out = f;
        return SDMM_OK;
    }
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void**)&f->final_d, sizeof(float) * n3);
    if (e == hipSuccess && mode == kFilmMaxVar) e = hipMalloc((void**)&f->recip_plane_d, sizeof(float) * n3);
    if (e == hipSuccess) e = hipMalloc((void**)&f->small_d, sizeof(double) * 8 + sizeof(float) * 4);
    if (e == hipSuccess) e = hipMemset(f->small_d, 0, sizeof(double) * 8 + sizeof(float) * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&f->p0, sizeof(double) * film_partials_doubles(f->npix, 0));
    if (e == hipSuccess) e = hipMalloc((void**)&f->p1, sizeof(double) * film_partials_doubles(f->npix, 1));
    if (e != hipSuccess) {
        free_device(f);
        delete f;
        return fail(SDMM_E_HIP, std::string("sdmm_film_create: ") + hipGetErrorString(e));
    }
    *out = f;
    return SDMM_OK;
}

void sdmm_film_destroy(sdmm_film* f) {
    if (!f) return;
    free_device(f);
    delete f;
}

int sdmm_film_add_pass(sdmm_film* f, const float* image, const float* image_sqr, int spp, int iteration,
                       void* hip_stream, sdmm_film_stats* pass_stats) {
    if (!f) return fail(SDMM_E_INVALID, "sdmm_film_add_pass: NULL film");
    if (!image || !image_sqr) return fail(SDMM_E_INVALID, "sdmm_film_add_pass: NULL image");
    if (spp < 2) return fail(SDMM_E_INVALID, "sdmm_film_add_pass: spp < 2 (the variance divides by spp - 1)");
    const FilmPassDev p = pass_of(f, image, image_sqr, spp);
    const int included = iteration >= f->first_iteration ? 1 : 0;
    const bool first = f->n_included == 0;
    const float wu = film_uniform_weight(spp);
    Pass rec{iteration, spp, included, {0.0, 0.0, 0.0, 0.0}};
    try {
        f->passes.reserve(f->passes.size() + 1);
    } catch (const std::bad_alloc&) {
        return fail(SDMM_E_NOMEM, "out of host memory");
    }
    if (f->device < 0) {
        try {
            host_var_reduce(f, p, rec.v);
        } catch (const std::bad_alloc&) {
            return fail(SDMM_E_NOMEM, "out of host memory");
        }
        if (included) host_accumulate(f, p, rec.v, wu, first);
    } else {
        hipStream_t st = (hipStream_t)hip_stream;
        HIP_TRY(hipSetDevice(f->device));
        const size_t i = f->passes.size();
        if (i / kHistBlock == f->hist_d.size()) {
            double* blk = nullptr;
            HIP_TRY(hipMalloc((void**)&blk, sizeof(double) * 4 * kHistBlock));
            try {
                f->hist_d.push_back(blk);
            } catch (const std::bad_alloc&) {
                (void)hipFree(blk);
                return fail(SDMM_E_NOMEM, "out of host memory");
            }
        }
        const FilmFinishDev fd{f->small_d, f->hist_d[i / kHistBlock] + 4 * (i % kHistBlock),
                               included && f->mode == kFilmVar ? f->recip3_d() : nullptr, f->npix, first ? 1 : 0, 0};
        f->last_stream = st;
        HIP_TRY(launch_film_var_reduce(p, f->p0, f->p1, fd, st));
        if (included)
            HIP_TRY(launch_film_accumulate(p, f->mode, f->small_d, wu, first ? 1 : 0, f->final_d, f->recip_plane_d,
                                           st));
    }
    if (included) {
        if (f->mode == kFilmUniform) f->recip_uniform += 1.0 / (1.0 / (double)spp);
        ++f->n_included;
    }
    f->passes.push_back(rec);
    if (f->device < 0) f->fetched = f->passes.size();
    if (pass_stats) {
        const int rc = fetch_history(f);
        if (rc) return rc;
        fill_stats(f->passes.back(), pass_stats);
    }
    return SDMM_OK;
}

int sdmm_film_passes(const sdmm_film* f) { return f ? (int)f->passes.size() : -1; }

int sdmm_film_pass_stats(sdmm_film* f, int i, sdmm_film_stats* out) {
    if (!f || !out) return fail(SDMM_E_INVALID, "sdmm_film_pass_stats: NULL argument");
    if (i < 0 || (size_t)i >= f->passes.size()) return fail(SDMM_E_INVALID, "sdmm_film_pass_stats: no such pass");
    const int rc = fetch_history(f);
    if (rc) return rc;
    fill_stats(f->passes[(size_t)i], out);
    return SDMM_OK;
}

int sdmm_film_resolve(sdmm_film* f, float* out, void* hip_stream) {
    if (!f || !out) return fail(SDMM_E_INVALID, "sdmm_film_resolve: NULL argument");
    if (f->n_included == 0) return fail(SDMM_E_STATE, "sdmm_film_resolve: no included pass yet");
    const FilmRecip r = f->recip();
    if (f->device < 0) {
        for (int ch = 0; ch < 3; ++ch)
            for (int64_t i = 0; i < f->npix; ++i) {
                const int64_t at = (int64_t)ch * f->npix + i;
                out[at] = film_resolve(f->final_h[at], film_recip_at(r, ch, f->npix, i));
            }
        return SDMM_OK;
    }
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(launch_film_resolve(f->final_d, r, f->npix, out, (hipStream_t)hip_stream));
    return SDMM_OK;
}

int sdmm_film_errors(sdmm_film* f, const float* image, const float* ground_truth, void* hip_stream,
                     sdmm_film_error* out) {
    if (!f || !ground_truth || !out) return fail(SDMM_E_INVALID, "sdmm_film_errors: NULL argument");
    if (!image && f->n_included == 0) return fail(SDMM_E_STATE, "sdmm_film_errors: no included pass yet");
    double v[3];
    if (f->device < 0) {
        try {
            host_errors(f, image, ground_truth, v);
        } catch (const std::bad_alloc&) {
            return fail(SDMM_E_NOMEM, "out of host memory");
        }
    } else {
        hipStream_t st = (hipStream_t)hip_stream;
        HIP_TRY(hipSetDevice(f->device));
        const FilmFinishDev fd{f->small_d + 4, nullptr, nullptr, f->npix, 0, 1};
        HIP_TRY(launch_film_errors(image, f->final_d, f->recip(), ground_truth, f->npix, f->p0, f->p1, fd, st));
        const int rc = read_back(v, f->small_d + 4, sizeof v, st);
        if (rc) return rc;
    }
    out->mrse = v[0];
    out->mape = v[1];
    out->smape = v[2];
    return SDMM_OK;
}

int sdmm_film_variance(const sdmm_film* f, const float* image, const float* image_sqr, int spp, float* out,
                       void* hip_stream) {
    if (!f || !image || !image_sqr || !out) return fail(SDMM_E_INVALID, "sdmm_film_variance: NULL argument");
    if (spp < 2) return fail(SDMM_E_INVALID, "sdmm_film_variance: spp < 2 (the variance divides by spp - 1)");
    const FilmPassDev p = pass_of(f, image, image_sqr, spp);
    if (f->device < 0) {
        for (int64_t i = 0; i < 3 * f->npix; ++i) out[i] = film_variance(image[i], image_sqr[i], p.fspp, p.coef);
        return SDMM_OK;
    }
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(launch_film_variance(p, out, (hipStream_t)hip_stream));
    return SDMM_OK;
}

int sdmm_film_reset(sdmm_film* f) {
    if (!f) return fail(SDMM_E_INVALID, "sdmm_film_reset: NULL film");
    if (f->device >= 0) {
        HIP_TRY(hipSetDevice(f->device));
        HIP_TRY(hipStreamSynchronize(f->last_stream));
    }
    f->passes.clear();
    f->fetched = 0;
    f->n_included = 0;
    f->recip_uniform = 0.0;
    return SDMM_OK;
}

}  // extern "C"
