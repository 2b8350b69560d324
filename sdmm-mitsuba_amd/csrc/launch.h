// launch.h -- the host-callable functions that the E-step, mstep.hip, guide.hip
// and stree.hip define for other translation units, declared once (render.hip's:
// render_launch.h): every defining file and every caller includes this header,
// default arguments appear here only, and the library links with --no-undefined.
#pragma once

#include "sdmm_device.h"

namespace sdmm {

// ---- estep.hip -------------------------------------------------------------
hipError_t launch_estep_resp(int cpl, int lps, const float* ep, int Kp, int K, const SamplesDev& s, int64_t n,
                             int64_t chunk, float* resp, hipStream_t st);
hipError_t launch_estep_stats(int cpl, int lps, const float* ep, int Kp, int K, const SamplesDev& s, int64_t n,
                              int64_t chunk, int blocks, int wpb, float* partials, int pstride, hipStream_t st,
                              const LeafDesc* leaves = nullptr, const int2* items = nullptr);
hipError_t estep_occupancy(int cpl, int lps, int Kp, int* resp_blocks, int* stats_blocks);
hipError_t launch_estep_resp_tile(const float* ep, int Kp, int K, const SamplesDev& s, int64_t n, int64_t chunk,
                                  float* resp, hipStream_t st);
hipError_t estep_resp_tile_occupancy(int* blocks_per_cu);
const char* estep_resp_tile_name();
hipError_t launch_estep_stats_tile(const float* ep, int Kp, int K, const SamplesDev& s, int64_t n, int64_t chunk,
                                   int blocks, float* partials, int pstride, hipStream_t st,
                                   const LeafDesc* leaves = nullptr, const int2* items = nullptr);
hipError_t estep_stats_tile_occupancy(int Kp, int* blocks_per_cu);
hipError_t launch_reduce_partials(const float* partials, int rows, int pstride, const float* ep_for_finalize, int Kp,
                                  int K, double* stats, hipStream_t st);
hipError_t launch_reduce_finalize_batched(const float* partials, int pstride, int Kp, int K, const LeafDesc* leaves,
                                          int n_leaves, hipStream_t st);

// ---- estep_mfma.hip --------------------------------------------------------
hipError_t launch_estep_resp_mfma(const float* ep, int Kp, int K, const SamplesDev& s, int64_t n, int64_t chunk,
                                  float* resp, hipStream_t st);
hipError_t estep_resp_mfma_occupancy(int Kp, int* blocks_per_cu);
const char* estep_resp_mfma_name(int Kp);

// ---- estep_split.hip (lds_image: the coefficient image in LDS at Kp = 128) --
bool estep_resp_split_supported(int Kp);
size_t estep_resp_image_bytes(int Kp);
hipError_t launch_estep_resp_image(const float* ep, int Kp, void* img, hipStream_t st);
hipError_t launch_estep_resp_split(bool lds_image, const float* ep, const void* img, int Kp, int K,
                                   const SamplesDev& s, int64_t n, int64_t resident_waves, float* resp,
                                   hipStream_t st);
hipError_t estep_resp_split_occupancy(bool lds_image, int Kp, bool inline_image, int* waves_per_cu);
const char* estep_resp_split_name(bool lds_image, int Kp, bool inline_image);

// ---- mstep.hip -------------------------------------------------------------
hipError_t launch_mstep(int K, int Kp, const double* stats, int64_t nSamples, const CanonDev& C, const EmStateDev& S,
                        float* ep, float* gp, float norm5, double* newW, unsigned* count, hipStream_t st);
hipError_t launch_mstep_batched(int K, int Kp, const MixDesc* mixes, int n_mix, float norm5, hipStream_t st);
hipError_t launch_set_f64(double* p, double v, hipStream_t st);
hipError_t launch_set_all(int K, int Kp, const double* mean, const double* cov, const CanonDev& C, float* ep,
                          float* gp, float norm5, hipStream_t st);
hipError_t launch_pack_all(int K, int Kp, const CanonDev& C, float* ep, float* gp, float norm5, hipStream_t st);
hipError_t launch_init_state(int K, const double* scal, const float* bprior, float eps, double* sc, float* bp,
                             float* bd, hipStream_t st);
hipError_t launch_init_pack_many(int n, int K, int Kp, const double* scal, const float* bprior, float eps, double* sc,
                                 float* bp, float* bd, const CanonDev& C, float* ep, float* gp, float norm5,
                                 size_t stride, hipStream_t st);
hipError_t launch_hemi_gen_batched(int n, int K, const float* pos, const float* nrm, const float* dist,
                                   const uint64_t* seed, int skip, float depth_prior, char* staging, size_t per,
                                   hipStream_t st);
hipError_t launch_set_all_batched(int n, int K, int Kp, const InitDesc* tab, const char* staging, size_t per,
                                  float norm5, hipStream_t st);
hipError_t launch_copy_many(int n, const uint4* const* src_tab, uint4* const* dst_tab, size_t bytes, hipStream_t st);
hipError_t launch_gather_f64(const double* const* src_tab, int n, double* out, hipStream_t st);

// ---- guide.hip -------------------------------------------------------------
// candidate-list capacity of the guided queries: the compiled maximum and the
// default (40: round 4 A/B, Cornell K=128 tree wavefront: 12.3 ms per guided
// pass at 40 against 13.3 ms at 64 -- a third of the fallback queries but 2
// instead of 3 waves per SIMD; K=512 product 92.2 vs 91.4 ms; the single
// K=128 mixture 613 vs 816 us)
#ifndef SDMM_GUIDE_CAP_MAX
#define SDMM_GUIDE_CAP_MAX 64
#endif
constexpr int kGuideCapMax = SDMM_GUIDE_CAP_MAX;
#ifndef SDMM_GUIDE_CAP_DEFAULT
#define SDMM_GUIDE_CAP_DEFAULT 40
#endif
constexpr int kGuideCapDefault = SDMM_GUIDE_CAP_DEFAULT;

size_t guide_sort_temp_bytes(int n);
hipError_t launch_guide(const float* gp, int Kp, int K, int64_t nq, const float* const c[3], const float* const u[3],
                        const float* const dgiven[3], float* const d[3], float* pdf, int32_t* comp, float norm2,
                        float norm3, int cap, int* fb_count, int32_t* fb_list, int cus, hipStream_t st,
                        const GuideSortScratch* sort, int* fb2 = nullptr);
hipError_t launch_guide_tree(const STNodeDev* nd, const GuideMix* tb, int kmax, int64_t nq, const float* const c[3],
                             const float* const u[3], const float* const dgiven[3], float* const d[3], float* pdf,
                             int32_t* comp, int32_t* node_out, float norm2, float norm3, int cap, int* fb_count,
                             int32_t* fb_list, int cus, hipStream_t st, const GuideSortScratch* sort,
                             const uint8_t* pmode = nullptr, int* fb2 = nullptr, int nn = 0);
hipError_t launch_guide_product(const float* gp, int Kp, int K, const float* condCov, int64_t nq,
                                const float* const c[3], const float* const u[3], const float* const dgiven[3],
                                float* const d[3], float* pdf, int32_t* comp, const int32_t* material,
                                const float* const frame[9], float* h, const float* bw, const float* bmean,
                                const float* bcov, const uint8_t* diffuse, int B, int M, float norm2, float norm3,
                                int cap, int* fb_count, int32_t* fb_list, int cus, hipStream_t st,
                                const GuideSortScratch* sort, ProductScratch* scratch);
hipError_t launch_guide_product_tree(const STNodeDev* nd, const GuideMix* tb, const float* const* cc, int kmax,
                                     int64_t nq, const float* const c[3], const float* const u[3],
                                     const float* choice, const float* const dgiven[3], float* const d[3], float* pdf,
                                     int32_t* comp, int32_t* node_out, const int32_t* material,
                                     const float* const frame[9], float* h, const float* bw, const float* bmean,
                                     const float* bcov, const uint8_t* diffuse, int B, int M, float norm2,
                                     float norm3, int cap, int* fb_count, int32_t* fb_list, int cus, hipStream_t st,
                                     const GuideSortScratch* sort, ProductScratch* scratch, int nn = 0);
hipError_t launch_sample_cdf(const float* cdf, int n, const float* u, int64_t nq, int32_t* out, hipStream_t st);

// ---- stree.hip -------------------------------------------------------------
hipError_t launch_stree_find(const STNodeDev* nodes, int64_t n, const float* p0, const float* p1, const float* p2,
                             int32_t* out, hipStream_t st);
size_t stree_route_temp_bytes(int n, int key_bits);
hipError_t launch_stree_route(const STNodeDev* nodes, int num_nodes, int key_bits, const SamplesDev& in, int n,
                              uint32_t* keys0, uint32_t* keys1, int32_t* idx0, int32_t* idx1, void* temp,
                              size_t temp_bytes, int64_t* seg_dev, float* const out_x[6], float* out_w, float* out_h,
                              uint8_t* out_d, hipStream_t st);
hipError_t launch_split_load(const float* const p[3], const int64_t* src_start, const int64_t* dst_start, int n_items,
                             int64_t total, float* ox, float* oy, float* oz, int32_t* oitem, hipStream_t st);
hipError_t launch_split_sums(const float* x, const float* y, const float* z, const SplitChunkDev* chunks,
                             int n_chunks, double* partial, hipStream_t st);
hipError_t launch_split_flags(const float* x, const float* y, const float* z, const int32_t* item, int64_t n,
                              const SplitCandDev* cand, int n_items, int32_t* flags, int64_t* rank, void* temp,
                              size_t temp_bytes, long long* counts, hipStream_t st);
hipError_t launch_split_scatter(const float* x, const float* y, const float* z, const int32_t* item, int64_t n,
                                const SplitCandDev* cand, const int32_t* flags, const int64_t* rank, float* ox,
                                float* oy, float* oz, int32_t* oitem, hipStream_t st);
hipError_t launch_split_decide(const SplitItemDev* items, int n_items, const double* partial, int threshold,
                               SplitCandDev* cand, SplitDecisionDev* dec, hipStream_t st);
size_t split_scan_temp_bytes(int64_t n);
int split_chunk_samples();

}  // namespace sdmm
