// render_launch.h -- the host-callable functions render.hip and film.hip define
// for other translation units, declared once (see launch.h).
#pragma once

#include "sdmm_device.h"
#include "render_device.h"
#include "film.h"

namespace sdmm {

// N: the vertex normals' record (N.shade null: none, the kernels' other variants run and read nothing of it)
// T: the textures' record (T.bsdf_tex null: no BSDF is textured, likewise)
hipError_t launch_li_camera(const SceneDev& S, const PathsDev& P, const NormalsDev& N, const TexDev& T, int64_t path0,
                            int spp, uint64_t seed, hipStream_t st);
hipError_t launch_li_query(const SceneDev& S, const PathsDev& P, const QueryDev& Q, const NormalsDev& N,
                           const TexDev& T, int64_t path0, int bounce, int max_depth, int guided, float h,
                           uint64_t seed, hipStream_t st);
hipError_t launch_li_shade(const SceneDev& S, const PathsDev& P, const QueryDev& Q, const NormalsDev& N,
                           const TexDev& T, int64_t path0, int bounce, int rr_depth, float h, uint64_t seed,
                           int product, hipStream_t st);
size_t li_select_temp_bytes(int64_t n);
hipError_t launch_li_compact(const SceneDev& S, const PathsDev& P, const QueryDev& Q, const NormalsDev& N, int64_t n,
                             int32_t* count_dev, void* temp, size_t temp_bytes, int product, hipStream_t st);
hipError_t launch_li_film(const PathsDev& P, int64_t pix0, int64_t npix, int spp, int64_t plane, float* image,
                          float* image_sqr, hipStream_t st);
hipError_t launch_scene_intersect(const SceneDev& S, int64_t nq, const float* const o[3], const float* const d[3],
                                  float mint, float maxt, int mode, int32_t* prim, float* t, hipStream_t st);
hipError_t launch_scene_shading(const SceneDev& S, const MeshShade* shade, int64_t nq, const float* const o[3],
                                const float* const d[3], float mint, float maxt, int mode, int32_t* prim, float* t,
                                float* const ns[3], float* const ng[3], hipStream_t st);
hipError_t launch_scene_texture(const SceneDev& S, const TexDev& T, int64_t nq, const float* const o[3],
                                const float* const d[3], float mint, float maxt, int mode, int32_t* prim, float* t,
                                float* const uv[2], float* const rgb[3], hipStream_t st);
hipError_t launch_env_eval(const SceneDev& S, int64_t nq, const float* const d[3], float* const rgb[3],
                           hipStream_t st);
hipError_t launch_roughdielectric(const float* bp, const float st[3], int64_t nq, const float* const wi[3],
                                  const float* const* u, float* const wo[3], float* const value[3], float* pdf,
                                  float* eta_out, hipStream_t st_);
hipError_t launch_smooth(const float* bp, const float st[3], int64_t nq, const float* const wi[3],
                         const float* const* u, float* const wo[3], float* const value[3], float* pdf,
                         float* eta_out, hipStream_t st_);
hipError_t launch_learned4(const float* rec, int M, float alpha, int64_t nq, const float* const wl[3], int keep,
                           float* w, float* mean, float* cov, int32_t* n, hipStream_t st);
hipError_t launch_learned_nd(int C, const float* rec, int M, const float* const* rest, const float* scal, int64_t nq,
                             const float* const wl[3], int keep, int force, float* w, float* mean, float* cov,
                             int32_t* n, hipStream_t st);

// training records of a render's paths, routed to the spatial tree's leaves
size_t produce_temp_bytes(int64_t n_paths, int64_t n_records, int key_bits);
hipError_t launch_produce_count(const STNodeDev* nodes, const PathsDev& P, int64_t path0, int saved, uint64_t seed,
                                int64_t* count, int64_t* offsets, void* temp, size_t temp_bytes, hipStream_t st);
hipError_t launch_produce_records(const STNodeDev* nodes, int num_nodes, int key_bits, const PathsDev& P,
                                  int64_t path0, int saved, uint64_t seed, const int64_t* offsets, int64_t n_rec,
                                  uint32_t* keys0, uint32_t* keys1, int64_t* codes0, int64_t* codes1, void* recs,
                                  void* temp, size_t temp_bytes, int64_t* seg_dev, int* lost, float* const x[6],
                                  float* const nrm[3], float* w, uint8_t* stats, int32_t* node, int64_t* source,
                                  hipStream_t st);

// ---- film.hip --------------------------------------------------------------
// scratch of a film's reductions, in doubles: which = 0 the chunk partials
// (p0), 1 the next level (p1); sized for the nine rows of the error sums
size_t film_partials_doubles(int64_t npix, int which);
// the pass's variance sums -> f.rec / f.hist (and f.recip3), two launches
hipError_t launch_film_var_reduce(const FilmPassDev& p, double* p0, double* p1, const FilmFinishDev& f,
                                  hipStream_t st);
// final (+)= img / w; rec: the device record launch_film_var_reduce wrote
hipError_t launch_film_accumulate(const FilmPassDev& p, int mode, const double* rec, float wu, int first,
                                  float* final_, float* recip_plane, hipStream_t st);
hipError_t launch_film_resolve(const float* final_, const FilmRecip& r, int64_t npix, float* out, hipStream_t st);
// image NULL: the combined estimate final_ / r
hipError_t launch_film_errors(const float* image, const float* final_, const FilmRecip& r, const float* truth,
                              int64_t npix, double* p0, double* p1, const FilmFinishDev& f, hipStream_t st);
hipError_t launch_film_variance(const FilmPassDev& p, float* out, hipStream_t st);

}  // namespace sdmm
